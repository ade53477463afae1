"""CPU checks of the cases and of the numpy model of the ordered scatter (tests/grid_ordered_cases.py): what the GPU tests rely on is
asserted here from numpy and the oracle alone -- every contribution of every lattice case is exactly representable in fp32; the model's
float64 terms agree with the oracle's backward; the model's order is a real order (another one gives other bits); the one-cell batch goes
through at least two further arrays of partial sums; the fp16 cases stay finite."""
import numpy as np
import pytest

import grid_ordered_cases as goc
import oracle

LATTICE = [(name, order, fp16, one_cell) for name in goc.LATTICE_NAMES for order in (1, 2) for fp16 in (False, True) for one_cell in (False, True)]


@pytest.mark.parametrize('name,order,fp16,one_cell', LATTICE)
def test_lattice_contributions_are_exact_in_fp32(name, order, fp16, one_cell):
    case = goc.lattice_case(name, order, fp16, one_cell)
    tab = case['tab']
    assert goc.fits_fp32(case['contrib'])
    assert order == 2 or one_cell or np.count_nonzero(case['contrib']) > 0.9 * case['contrib'].size   # (order 2: sum_d +-u_d may vanish)
    assert goc.fits_fp32(case['g'].astype(np.float64))
    if fp16:
        # what an fp16 call is given (the gradient and u in the table dtype) and what it adds up stay finite in fp16
        assert np.array_equal(oracle.round_fp16(case['g']), case['g'])
        assert case['u'] is None or np.array_equal(oracle.round_fp16(case['u']), case['u'])
        _, a = goc.exact_sum(case['keys'], case['contrib'], case['size'], tab['C'])
        assert a.max() < 6e4
    if order == 2:
        assert np.array_equal(oracle.round_fp16(case['g']), case['g'])   # a_k g fits 24 bits only with 11-bit gradients
    if not one_cell:
        assert case['x'][40, 0] > 1.0 and (case['keys'].reshape(-1, 1 << tab['D'])[40] == goc.NONE).all()
    # every point sits at a cell centre of the lattice level: every first-order weight is 2^-D
    _, frac, inside = goc.level_position(case['x'], goc.level_scale(tab, case['level']), tab['align'])
    assert (frac[inside] == 0.5).all()


@pytest.mark.parametrize('name', goc.LATTICE_NAMES)
def test_first_order_terms_agree_with_the_oracle(name):
    """the model's float64 terms of every level, summed per entry, against the oracle's backward (fp32 weights, float64 sums)"""
    case = goc.lattice_case(name, 1, False)
    tab, x, g = case['tab'], case['x'], case['g']
    offs = tab['offs']
    ref, _ = oracle.grid_backward(g, x, offs, int(offs[-1]), tab['C'], tab['S'], tab['H'], gridtype=tab['gridtype'], align_corners=tab['align'],
                                  interp=tab['interp'])
    for level in range(tab['L']):
        size = int(offs[level + 1] - offs[level])
        keys = goc.record_keys(tab, x, level)
        s, a = goc.exact_sum(keys, goc.contributions(tab, x, g, level), size, tab['C'])
        assert np.abs(s - ref[offs[level]:offs[level + 1]]).max() <= 1e-6 * a.max()   # (the oracle's weight product is fp32)


def test_second_order_terms_agree_with_a_finite_difference():
    """a_k = d/dt w_k(x + t u) at t = 0: the model's coefficient against a central difference of its own first-order weights (smoothstep,
    general points)"""
    tab = goc.general_table(3, 2, interp=1)
    rng = np.random.default_rng(5)
    B = 64
    x = rng.uniform(0.05, 0.95, (B, 3)).astype(np.float32)
    u = (rng.uniform(0.5, 1.0, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))).astype(np.float32)
    g = np.ones((tab['L'], B, 2), np.float32)
    h = 2.0 ** -10
    for level in range(tab['L']):
        scale = goc.level_scale(tab, level)
        a = goc.contributions(tab, x, g, level, 2, u)
        # (the fp32 rounding of the displaced points moves them by 2^-24 / h of the step at most: far inside the tolerance)
        xp, xm = (x.astype(np.float64) + h * u).astype(np.float32), (x.astype(np.float64) - h * u).astype(np.float32)
        same_cell = (goc.level_position(xp, scale, False)[0] == goc.level_position(xm, scale, False)[0]).all(axis=1)
        fd = (goc.contributions(tab, xp, g, level) - goc.contributions(tab, xm, g, level)) / (2.0 * h)
        keep = np.repeat(same_cell, 8)
        assert keep.sum() > 100
        assert np.abs(a - fd)[keep].max() < 2e-3 * np.abs(a).max()


@pytest.mark.parametrize('name', goc.LATTICE_NAMES)
def test_the_order_shows_in_the_bits(name):
    """the comparison has teeth: the same fp32 contributions summed in reverse slot order change the bits of at least 40 % of the fp32 entries
    that receive 16 or more contributions (sequential fp32 sums of 16 such terms differ in 58 % (fp16-valued gradients) to 71 % (fp32 ones) of
    20000 simulated trials, more for longer runs)"""
    for order in (1, 2):
        case = goc.lattice_case(name, order, False)
        C = case['tab']['C']
        model, _ = goc.ordered_sum(case['keys'], case['contrib'], case['size'], C)
        other = goc.reversed_sum(case['keys'], case['contrib'], case['size'], C)
        many = goc.entry_counts(case['keys'], case['size']) >= 16
        assert many.sum() >= 8
        differ = (model.view(np.uint32) != other.view(np.uint32))[many]
        assert differ.mean() >= 0.4, (order, differ.mean())
        # ... and both are sums of the same terms
        s, a = goc.exact_sum(case['keys'], case['contrib'], case['size'], C)
        n = goc.entry_counts(case['keys'], case['size'])[:, None]
        assert (np.abs(model - s) <= n * 2.0 ** -24 * a).all() and (np.abs(other - s) <= n * 2.0 ** -24 * a).all()


def test_the_model_on_arrays_small_enough_to_state_by_hand():
    f = np.float32
    # one run of 3 inside a tile: ((a + b) + c)
    a, b, c = f(1.0), f(2.0 ** -24), f(2.0 ** -24)
    got, arrays = goc.ordered_sum(np.array([5, 5, 5]), np.array([[a], [b], [c]], np.float64), 8, 1)
    assert arrays == 1 and got[5, 0] == f(f(a + b) + c) == f(1.0) and f(a + f(b + c)) != f(1.0)
    # a run of 130 records of one entry: tiles of 64, 64 and 2 records; the first tile's fragment crosses right (slot 1), the second both
    # (slot 2, slot 3 repeats the entry), the third left (slot 4); the next array [-, p0, p1, (p1), p2, -] is one tile: (p0 + p1) + p2
    v = np.exp2(np.arange(130) % 31 - 15.0) * (1 + 2.0 ** -23)
    got, arrays = goc.ordered_sum(np.full(130, 3), v[:, None], 4, 1)
    seq = lambda w: np.cumsum(w.astype(f), dtype=f)[-1]
    assert arrays == 2 and got[3, 0] == f(f(seq(v[:64]) + seq(v[64:128])) + seq(v[128:]))
    # records of points outside sort last and add nothing; the sort is stable
    got, _ = goc.ordered_sum(np.array([goc.NONE, 1, 0, 1, goc.NONE]), np.array([[9.0], [1.0], [4.0], [2.0 ** -24], [9.0]]), 2, 1)
    assert got[:, 0].tolist() == [4.0, 1.0]
    # an entry that already holds a value: dst = T(float32(dst) + sum), fp16 rounds once at the end
    dst = np.full((1, 1), 0.5, np.float16)
    goc.ordered_sum(np.zeros(4, np.int64), np.full((4, 1), 2.0 ** -13), 1, 1, np.float16, dst)
    assert dst[0, 0] == np.float16(0.5 + 2.0 ** -11)


@pytest.mark.parametrize('name', ('A2', 'A5'))
def test_one_cell_batch_needs_two_further_arrays(name):
    case = goc.lattice_case(name, 1, False, True)
    counts = goc.entry_counts(case['keys'], case['size'])
    assert counts.max() >= goc.B_ONE_CELL > 64 * 64
    _, arrays = goc.ordered_sum(case['keys'], case['contrib'], case['size'], case['tab']['C'])
    assert arrays >= 3
