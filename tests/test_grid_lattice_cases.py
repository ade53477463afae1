"""The lattice inputs of tests/test_gpu_grid_backward_runs.py are what they claim to be (tests/grid_lattice_cases.py): conditions on the
INPUTS, from the CPU oracle alone, for every case the GPU tests use.  Exact sums, long runs, collisions, dead samples inside runs."""
import numpy as np
import pytest

import oracle

import grid_lattice_cases as glc


@pytest.mark.parametrize('case', glc.ALL_CASES, ids=glc.case_id)
def test_case_is_exact_and_has_the_run_structure(case):
    x, g, offs, S = glc.make(case)
    e = glc.exactness(case)
    T = np.float16 if case.dtype == 'f16' else np.float32
    assert S == 0.0 and x.shape == (case.B, case.D) and g.shape == (len(case.level_sizes), case.B, case.C)
    assert case.B % 64 != 0 and case.B % 128 != 0
    # the points are on the lattice, exactly
    assert np.array_equal(e['lattice'], np.rint(e['lattice']))
    assert (~e['inside']).sum() >= 0.02 * case.B
    out = x[~e['inside']]
    assert (out == np.nextafter(np.float32(1), np.float32(2))).any() and (out == np.float32(-1e-7)).any()
    assert (x == 0).all(1).any() and (x == 1).all(1).any()
    # the gradients are small integers times 2^-6
    j = g.astype(np.float64) * 64
    assert np.array_equal(j, np.rint(j)) and np.abs(j).max() <= case.jmax
    # every sum is an integer multiple of the unit and stays below the cap, the "+=" start value included
    q = e['ref'] / e['unit']
    assert np.array_equal(q, np.rint(q))
    assert (glc.PREFILL + e['A'].max()) / e['unit'] < e['cap']
    assert np.array_equal(e['ref'].astype(T).astype(np.float64), e['ref'])
    assert np.array_equal((glc.PREFILL + e['ref']).astype(T).astype(np.float64), glc.PREFILL + e['ref'])
    assert np.all(e['A'][e['hits'] == 0] == 0) and np.all(e['A'] >= np.abs(e['ref']))
    # long runs, dead and zero-gradient samples inside runs
    assert e['runs'].max() >= 100
    assert (e['runs'] > 8).sum() >= 50
    assert all((r > 8).sum() >= 50 and r.max() >= 100 for r in e['vertex_runs']), 'in every slot of the merge'
    for n in (8, 9, 16, 17, 32):
        assert (e['runs'] == n).any(), n
    assert e['dead_in_run'] >= 2 and e['zero_in_run'] >= 1
    if case.C > 1:
        assert e['partial_zero_in_run'] >= 1
    # hashed levels: different vertices share an address
    for l in glc.hashed_levels(case):
        assert e['collisions'][l] >= 1, l
    # every level takes part
    for l in range(len(case.level_sizes)):
        assert np.any(e['ref'][offs[l]:offs[l + 1]] != 0)


def test_layout_cases_cover_every_instantiation_and_mode():
    cases = glc.LAYOUT_CASES
    assert len({(c.dtype, c.C, c.D) for c in cases}) == 32
    assert {glc.lanes_per_point(c.dtype, c.C) for c in cases} == {2, 4, 8, 16}
    for dtype in ('f16', 'f32'):
        for merge in (1, 3):
            grp = [c for c in cases if c.dtype == dtype and glc.merge_kind(dtype, c.C) == merge]
            assert any(glc.hashed_levels(c) for c in grp), 'hash'
            assert any(c.gridtype == 0 and not glc.hashed_levels(c) for c in grp), 'dense'
            assert any(c.gridtype == 1 and c.level_sizes[0] < glc.dense_size(c.D, c.H, c.align) for c in grp), 'tiled, wrapping'
            assert any(c.align for c in grp), 'align_corners'
            assert any(c.interp == 1 for c in grp), 'smoothstep'
    assert all(c.sub == 2 for c in cases if c.interp == 1 or c.dtype == 'f16')


def test_sweep_cases_have_three_different_levels():
    assert len(glc.SWEEP_CASES) == 16
    assert len({(c.dtype, c.gridtype, c.align, c.interp) for c in glc.SWEEP_CASES}) == 16
    for c in glc.SWEEP_CASES:
        assert c.level_sizes[2] == 8 and c.level_sizes[1] >= (c.H if c.align else c.H + 1) ** 3 > c.level_sizes[0]


def test_world_coordinates_map_back_exactly():
    """(xw + bound) * (1 / (2 bound)) in fp32 gives the unit lattice point back, bit for bit, and keeps both kinds of outside point outside"""
    for case in glc.MAPPED_CASES:
        x, _, _, _ = glc.make(case)
        xw = glc.world_coordinates(x)
        back = (xw + np.float32(glc.BOUND)) * np.float32(1.0 / (2.0 * glc.BOUND))
        inside = glc.exactness(case)['inside']
        assert back.dtype == np.float32 and np.array_equal(back[inside], x[inside])
        assert np.all(np.any((back[~inside] < 0) | (back[~inside] > 1), axis=1))


@pytest.mark.parametrize('D,C,dtype,gridtype,align,interp,log2_size', glc.RAY_CASES)
def test_ray_cases_have_long_hit_lists_and_normal_fp16_contributions(D, C, dtype, gridtype, align, interp, log2_size):
    rc = glc.ray_case(D, C, dtype, gridtype, align, interp, log2_size)
    x, g, A, hits = rc['x'], rc['g'], rc['A'], rc['hits']
    assert x.shape == (4096, D) and g.shape == (3, 4096, C)
    assert hits.max() >= 64 and (hits == 0).any() and np.all(A[hits == 0] == 0)
    assert np.all(A >= np.abs(rc['ref']))
    if dtype == 'f16':
        assert np.array_equal(g, oracle.round_fp16(g)) and np.abs(g).max() <= 32 and np.abs(g[g != 0]).min() >= 16
        # every contribution is a normal fp16 number: weight >= 2^-18 wherever it is not zero, |g| >= 16; only a few samples paid for it
        assert A[A > 0].min() >= glc.FP16_MIN_NORMAL
        assert 0 < rc['zeroed'] <= 0.01 * 3 * 4096
        assert A.max() < 65504 / 4
    assert {c[5] for c in glc.RAY_CASES} == {0, 1} and {c[3] for c in glc.RAY_CASES} == {0, 1} and {c[4] for c in glc.RAY_CASES} == {False, True}


@pytest.mark.parametrize('name,level', [('T3', 1), ('T1', 0)])
def test_level_lattice_inputs_are_exact_at_their_level(name, level):
    """the inputs of tests/test_gpu_grid_backward_paths.py for calls with an atomic level: positions exactly on the half lattice of that level
    (whose scale is no power of two), sums there in multiples of the unit and below the fp16 cap, runs longer than a DPP row"""
    import grid_backward_path_cases as pc
    tab = pc.table(name)
    scale = np.float32(pc.level_scale(tab, level))
    for B in pc.BATCHES:
        x, g = pc.lattice_inputs(name, B, level)          # (asserts level_lattice_exact)
        inside = np.all((x >= 0) & (x <= 1), axis=1)
        pos = (x[inside].astype(np.float64) * float(scale) + 0.5).astype(np.float32).astype(np.float64)
        assert np.array_equal(pos * 2, np.rint(pos * 2)) and (~inside).sum() == 1
        units = g[level] / 2.0 ** -6
        assert np.array_equal(units, np.rint(units)) and np.abs(units).max() == 2 and (units == 0).all(axis=1).mean() > 0.02
        same = np.all(x[1:] == x[:-1], axis=1)
        run = best = 0
        for s in same:
            run = run + 1 if s else 0
            best = max(best, run)
        assert best >= 129
        assert glc.level_lattice_exact(x, g[level], tab['offs'], level, tab['S'], tab['H']) > 64   # entries that many contributions meet in
