"""CPU checks of tests/occupancy_cases.py, the models and case tables of the occupancy kernels (tests/test_gpu_occupancy.py): the numpy coarse
model against the voxel-by-voxel oracle, the fp32 cull model's conservativeness against the marcher on every table and every dt_gamma, the
conditions the tables promise (layouts, duplicate groups that straddle blocks, no cell near the packing threshold, exactly summable dyadic
grids), and that the tables tell every deliberately wrong variant from its model."""
import math

import numpy as np
import pytest

import oracle
import occupancy_cases as O

F32 = np.float32


def test_every_listed_wrong_version_is_there():
    assert O.VARIANTS == dict(coarse=('no dilation', 'faces only', 'axes swapped'), cull=('step 1.8', 'lookup from lp', 'finest cascade only'),
                              update=('ema below zero', 'no decay', 'mean without clamp', 'ge packbits'))


# ---- coarse occupancy --------------------------------------------------------------------------------------------------------------------
def test_volumes_round_trip_and_follow_the_morton_order():
    rng = np.random.default_rng(0)
    vol = rng.random((2, 16, 16, 16)) < 0.1
    bits = O.pack_volumes(vol)
    assert np.array_equal(O.unpack_volumes(bits, 2, 16), vol)
    # against the oracle's own statement of the order: density [cascade, morton index] -> packbits
    dens = np.zeros((2, 16 ** 3), F32)
    c, z, y, x = np.nonzero(vol)
    dens[c, oracle.morton3D(np.stack([x, y, z], -1).astype(np.int32))] = 1.0
    assert np.array_equal(bits, oracle.packbits(dens.reshape(-1), 0.5))


@pytest.mark.parametrize('H,C', O.COARSE_GRIDS)
def test_coarse_model_equals_the_oracle_and_differs_from_every_wrong_variant(H, C):
    R = H // 4
    told = {v: False for v in O.COARSE_VARIANTS[1:]}
    for fill in O.COARSE_FILLS:
        bits = O.coarse_fill(fill, C, H)
        ref = O.coarse_model(bits, C, H)
        assert ref.shape == (C * R ** 3,) and ref.dtype == np.uint8 and set(np.unique(ref)) <= {0, 1}
        assert np.array_equal(oracle.coarse_occupancy(bits, C, H), ref), fill
        for v in told:
            told[v] |= not np.array_equal(O.coarse_model(bits, C, H, v), ref)
        vol = ref.reshape(C, R, R, R)                        # [c, z, y, x]
        if fill == 'empty':
            assert not ref.any()
        elif fill == 'full':
            assert ref.all()
        elif fill == 'first voxel':
            assert vol[:, :2, :2, :2].all() and vol.sum() == 8 * C
        elif fill == 'last voxel':
            assert vol[:, -2:, -2:, -2:].all() and vol.sum() == 8 * C
        elif fill == 'odd voxel':
            x, y, z = (a // 4 for a in O.odd_voxel(H))
            assert len({x, y, z}) == 3 and vol[0, z, y, x] and not vol[0, x, y, z]
        elif fill == '64 bits':
            u = O.unpack_volumes(bits, C, H).reshape(C, R, 4, R, 4, R, 4)
            per_block = u.sum(axis=(2, 4, 6))
            assert per_block.max() == 1 and (per_block.sum(axis=(1, 2, 3)) == 64).all()
            local = u.any(axis=(0, 1, 3, 5))                  # which of the 64 positions inside a block are used
            assert local.all()
    assert all(told.values()), told


# ---- ray cull ----------------------------------------------------------------------------------------------------------------------------
def test_named_rays_get_the_stated_verdict():
    bound, C, H = O.NAMED_GRID
    for fill in ('empty', 'full'):
        names, o, d, nears, fars, kept = O.named_rays(fill)
        assert len(names) >= 3
        flags = O.cull_model(o, d, nears, fars, bound, C, H, O.coarse_model(O.coarse_fill(fill, C, H), C, H))
        for i, name in enumerate(names):
            assert flags[i] == (i if kept[i] else -1), name
    assert sum(len(O.named_rays(f)[0]) for f in ('empty', 'full')) == len(O.NAMED_RAYS)


@pytest.mark.parametrize('bound,C,H', O.CULL_CONFIGS)
def test_cull_tables_have_the_stated_mix(bound, C, H):
    t = O.cull_table(bound, C, H)
    N = O.CULL_N
    assert t['o'].shape == (N, 3) and t['o'].dtype == F32 and t['d'].dtype == F32 and t['nears'].dtype == F32
    inside = (np.abs(t['o']) <= bound).all(axis=1)
    assert 0.3 * N <= inside.sum() <= 0.4 * N
    zero = (t['d'] == 0).any(axis=1)
    length = np.linalg.norm(t['d'].astype(np.float64), axis=1)
    assert zero.sum() >= 0.09 * N and ((t['d'] == 0).sum(axis=1) == 2).sum() >= 0.04 * N
    assert (length[zero] < 1 - 1e-3).sum() >= 0.08 * N                       # not renormalised
    assert (t['nears'] < t['fars']).sum() >= 0.8 * N and (t['nears'] >= t['fars']).sum() >= 1
    assert np.isfinite(t['d']).all() and np.isfinite(t['o']).all()
    flags = O.cull_model(t['o'], t['d'], t['nears'], t['fars'], bound, C, H, t['coarse'])
    kept = flags >= 0
    assert np.array_equal(flags[kept], np.arange(N, dtype=np.int32)[kept]) and (flags[~kept] == -1).all()
    assert kept.sum() >= 0.05 * N and (~kept).sum() >= 0.05 * N
    assert O.table_emits(bound, C, H, 0.0).sum() >= 0.02 * N                    # the aimed rays do hit


@pytest.mark.parametrize('bound,C,H', O.CULL_CONFIGS)
def test_cull_model_is_conservative_on_every_table(bound, C, H):
    """no ray the model drops emits a sample from the marcher (n_step = 1, t from near), at any dt_gamma: a CONDITION on the algorithm"""
    t = O.cull_table(bound, C, H)
    culled = O.cull_model(t['o'], t['d'], t['nears'], t['fars'], bound, C, H, t['coarse']) < 0
    for dt_gamma in O.DT_GAMMAS:
        bad = culled & O.table_emits(bound, C, H, dt_gamma)
        assert not bad.any(), (dt_gamma, int(bad.sum()), np.nonzero(bad)[0][:5])


def _variant_counts():
    """per wrong version: (flags that differ from the model's, culled rays that emit at some dt_gamma) summed over the tables"""
    out = {}
    for bound, C, H in O.CULL_CONFIGS:
        t = O.cull_table(bound, C, H)
        args = (t['o'], t['d'], t['nears'], t['fars'], bound, C, H)
        ref = O.cull_model(*args, t['coarse'])
        em = np.zeros(O.CULL_N, bool)
        for dt_gamma in O.DT_GAMMAS:
            em |= O.table_emits(bound, C, H, dt_gamma)
        versions = {v: O.cull_model(*args, t['coarse'], v) for v in O.CULL_VARIANTS[1:]}
        versions.update({'coarse: ' + v: O.cull_model(*args, O.coarse_model(t['bits'], C, H, v)) for v in O.COARSE_VARIANTS[1:]})
        for v, flags in versions.items():
            a, b = out.get(v, (0, 0))
            out[v] = (a + int((flags != ref).sum()), b + int(((flags < 0) & em).sum()))
    return out


def test_cull_tables_tell_every_wrong_version_from_the_model():
    counts = _variant_counts()
    print(counts)
    for v in O.CULL_VARIANTS[1:]:
        assert counts[v][0] > 0, (v, counts[v])
    for v in O.COARSE_VARIANTS[1:]:
        assert counts['coarse: ' + v][0] > 0, (v, counts)
    # these two do not merely differ: they drop rays that emit samples
    assert counts['lookup from lp'][1] > 0, counts
    assert counts['coarse: no dilation'][1] > 0, counts


# ---- density grid update -------------------------------------------------------------------------------------------------------------------
def test_fmax_hw_orders_the_zeros_and_drops_a_nan():
    a = np.array([0.0, -0.0, -0.0, 0.0, np.nan, 2.0, 1.0], F32)
    b = np.array([-0.0, 0.0, -0.0, 0.0, 1.0, np.nan, 3.0], F32)
    want = np.array([0.0, 0.0, -0.0, 0.0, 1.0, 2.0, 3.0], F32)
    assert np.array_equal(O.fmax_hw(a, b).view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('kind', O.UPDATE_KINDS)
@pytest.mark.parametrize('n_cells', O.UPDATE_CELLS)
def test_update_tables_have_the_stated_layout(kind, n_cells):
    t = O.update_table(kind, n_cells)
    g0 = t['grid0']
    assert g0.shape == (n_cells,) and g0.dtype == F32 and n_cells % 8 == 0
    assert (g0 < 0).any() and ((g0 == 0) & ~np.signbit(g0)).any() and ((g0 == 0) & np.signbit(g0)).any() and (g0 > 0).any()
    assert g0[0] == -1 and g0[3] == g0[g0 > 0].min() and g0[4] == g0.max() and (g0[5:8] > 0).all()
    (s0, c0), (s1, c1), (s2, c2), (s3, c3) = t['calls']
    for s, c in t['calls']:
        assert s.dtype == F32 and c.dtype == np.int64 and s.shape == c.shape and (c >= 0).all() and (len(c) == 0 or c.max() < n_cells + O.OOB)
    # call 0: every cell exactly once, the out-of-range indices n_cells .. n_cells + 7 in the middle
    assert sorted(c0.tolist()) == list(range(n_cells + O.OOB)) and (c0[n_cells // 2:n_cells // 2 + O.OOB] >= n_cells).all()
    f0 = dict(zip(c0.tolist(), (s0 * F32(t['scale'])).astype(F32).tolist()))
    sp = t['special']
    assert math.isnan(f0[sp['nan']]) and f0[sp['negative']] < 0
    for name in ('minus zero on zero', 'minus zero on minus zero'):
        assert f0[sp[name]] == 0 and math.copysign(1, f0[sp[name]]) < 0
    assert g0[sp['minus zero on zero']] == 0 and not np.signbit(g0[sp['minus zero on zero']]) and np.signbit(g0[sp['minus zero on minus zero']])
    cell = sp['equal to decayed']
    assert g0[cell] > 0 and F32(f0[cell]) == F32(g0[cell] * F32(t['decay']))
    # call 1: the duplicate groups, each in at least two of the scatter's 256-thread blocks, with different values
    assert sorted(t['groups']) == list(O.DUP_GROUPS)
    for copies, cell in t['groups'].items():
        pos = np.nonzero(c1 == cell)[0]
        assert len(pos) == copies and len(set((pos // O.SCATTER_THREADS).tolist())) >= 2, (copies, pos)
        assert len(set(s1[pos][~np.isnan(s1[pos])].tolist())) >= min(copies, 3) - 1
    others = c1[~np.isin(c1, list(t['groups'].values()))]
    assert len(set(others.tolist())) == len(others) and (c1 >= n_cells).sum() == O.OOB
    assert np.isnan(s1).sum() == 2 and (s1 < 0).sum() == 2
    assert len(c2) == 0
    assert np.isinf(s3).sum() == (0 if kind == 'dyadic' else 1) and (c3 >= n_cells).sum() == 2


@pytest.mark.parametrize('kind', O.UPDATE_KINDS)
@pytest.mark.parametrize('n_cells', O.UPDATE_CELLS)
def test_update_model_on_the_tables(kind, n_cells):
    t = O.update_table(kind, n_cells)
    ref = O.update_reference(kind, n_cells)
    grid = t['grid0']
    for i, ((sigmas, cells), r) in enumerate(zip(t['calls'], ref)):
        new = r['grid']
        sampled = np.zeros(n_cells, bool)
        sampled[r['sampled']] = True
        assert np.array_equal(new[~sampled].view(np.int32), grid[~sampled].view(np.int32))          # untouched cells keep their bits: no decay
        below = grid < 0
        assert np.array_equal(new[below].view(np.int32), grid[below].view(np.int32))                # cells < 0 are left alone
        # the first-wins grid lies within the admissible sets
        for cell, allowed in r['admissible'].items():
            assert int(new[cell:cell + 1].view(np.int32)[0]) in allowed
        if i == 1:
            assert sorted(r['admissible']) == sorted(t['groups'].values())
            big = r['admissible'][t['groups'][1000]]
            assert len(big) > (1 if grid[t['groups'][1000]] >= 0 and n_cells > 8 else 0)
        else:
            assert not r['admissible']
        assert np.isfinite(new).all() or (kind == 'generic' and i == 3)
        # the mean is the exact one
        assert r['mean'] == F32(math.fsum(np.maximum(new.astype(np.float64), 0).tolist()) / n_cells)
        if kind == 'dyadic':
            # multiples of 2^-13 below 128: any order of double additions is exact (2^21 cells x 2^7 x 2^13 = 2^41 < 2^53)
            scaled = new.astype(np.float64) * 2.0 ** 13
            assert np.array_equal(scaled, np.round(scaled)) and np.abs(new).max() < 128
            assert float(r['mean']) * n_cells == float(np.maximum(new.astype(np.float64), 0).sum()) or n_cells > 8
        else:
            # no cell within 4 ulp of the packing threshold: a mean that is 1 ulp off packs the same bits
            assert O.cells_near(new, min(F32(t['thresh']), r['mean'])) == 0, (i, r['mean'])
        assert np.array_equal(r['bitfield'], oracle.packbits(new, float(min(F32(t['thresh']), r['mean']))))
        grid = new
    sp = t['special']
    g0, g1 = t['grid0'], ref[0]['grid']
    for name in ('nan', 'negative'):                                                                # not applied: not even decayed
        assert g1[sp[name]] == g0[sp[name]] > 0
    assert g1[sp['minus zero on zero']] == 0 and not np.signbit(g1[sp['minus zero on zero']])
    assert g1[sp['minus zero on minus zero']] == 0 and np.signbit(g1[sp['minus zero on minus zero']])
    assert g1[sp['equal to decayed']] == F32(g0[sp['equal to decayed']] * F32(t['decay']))
    if kind == 'generic':
        assert np.isinf(ref[3]['grid']).sum() == 1 and np.isinf(ref[3]['mean'])
        thresh_decides = t['thresh'] < 1
        assert all((F32(t['thresh']) < r['mean']) == thresh_decides for r in ref[:3])


def test_update_tables_tell_every_wrong_version_from_the_model():
    for v in O.UPDATE_VARIANTS[1:]:
        for kind in O.UPDATE_KINDS:
            for n_cells in O.UPDATE_CELLS[:5]:
                t = O.update_table(kind, n_cells)
                ref, bad = O.update_reference(kind, n_cells), O.update_reference(kind, n_cells, v)
                differs = any(not np.array_equal(a['grid'].view(np.int32), b['grid'].view(np.int32)) or a['mean'] != b['mean'] or
                              not np.array_equal(a['bitfield'], b['bitfield']) for a, b in zip(ref, bad))
                # (`>=` shows where a cell EQUALS the packing threshold: in the dyadic tables in which the threshold decides)
                assert differs or (v == 'ge packbits' and (kind == 'generic' or t['thresh'] != O.DYADIC_THRESH or n_cells == 8)), (v, kind, n_cells)


def test_the_wrong_packbits_is_told_by_the_packbits_cases():
    told = 0
    for case in O.packbits_cases():
        ref = O.packbits_model(case['grid'], case['thresh'], case['cap'])
        cap = case['cap']
        t = case['thresh'] if cap is None or math.isnan(cap) else min(case['thresh'], cap)
        assert np.array_equal(ref, oracle.packbits(case['grid'], t)), case['name']
        assert len(ref) == len(case['grid']) // 8
        told += not np.array_equal(O.packbits_model(case['grid'], case['thresh'], cap, ge=True), ref)
        assert (case['grid'] == F32(t)).any() and (np.isnan(case['grid']).any() or len(ref) == 1)
    assert told == len(O.packbits_cases())
    g, T = O.packbits_f64_case()
    as64, as32 = O.packbits_model(g, T), O.packbits_model(g.astype(F32), T)
    assert not np.array_equal(as64, as32)                                                          # the double comparison is observable
