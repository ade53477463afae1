"""The numpy model of the error-map draw (tests/error_map_cases.py) draws the distribution include/ngp_hip.h states: successive sampling
without replacement proportional to the weights.  The z-scores use the binomial sigma of each inclusion count; they are conditions on the
MODEL (hash + exponential race), not on the GPU -- tests/test_gpu_error_map.py then pins the kernel to the model exactly.  Three wrong
draws (with replacement, unweighted, key = u / w) each fail one of the two checks, so the checks can tell."""
import numpy as np
import pytest

import error_map_cases as em

SMALL = np.array([1, 2, 3, 6, 0.5, 4], np.float32)
N_SMALL_SEEDS, Z_SMALL = 20000, 5.0
RES, N_BIG, N_BIG_SEEDS, Z_BIG = 128, 4096, 400, 5.5


def _small_z(fn):
    p = em.inclusion_probabilities_n2(SMALL)
    assert abs(p.sum() - 2.0) < 1e-12
    return max(np.abs(em.binomial_z(em.inclusion_counts(fn, SMALL, 2, b, range(N_SMALL_SEEDS)), N_SMALL_SEEDS, p)).max() for b in (0, 1))


@pytest.fixture(scope='module')
def big_counts():
    """per-cell inclusion counts of the uniform 16 384-cell map, N = 4096, 400 seeds: (model, with replacement)"""
    w = np.ones(RES * RES, np.float32)
    return em.inclusion_counts(em.draw, w, N_BIG, 0, range(N_BIG_SEEDS)), em.inclusion_counts(em.draw_with_replacement, w, N_BIG, 0, range(N_BIG_SEEDS))


def test_hash_words_and_uniforms():
    # the finaliser is seeded_noise's (raymarching.hip): the same integer steps on a known word
    x = 0x12345678
    y = x ^ (x >> 16); y = (y * 0x7FEB352D) & 0xFFFFFFFF; y ^= y >> 15; y = (y * 0x846CA68B) & 0xFFFFFFFF; y ^= y >> 16
    assert int(em.mix(x)) == y
    i = np.arange(4096)
    u = em.uniforms(i, 1, 7)
    assert u.min() > 0 and u.max() < 1 and np.array_equal(u.astype(np.float32).astype(np.float64), u)   # exact in fp32
    assert np.all((u * 2.0 ** 24).astype(np.int64) % 2 == 1)
    # streams, images and seeds are different words
    assert len({tuple(em.word(i, b, k, s).tolist()) for b in (0, 1) for k in (0, 1, 2) for s in (0, 1)}) == 12
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)


def test_small_map_inclusion_matches_successive_sampling():
    z = _small_z(em.draw)
    print('largest |z|, weights [1,2,3,6,0.5,4], N = 2:', z)
    assert z <= Z_SMALL


def test_uniform_map_inclusion_is_binomial(big_counts):
    counts = big_counts[0]
    assert counts.sum() == N_BIG * N_BIG_SEEDS
    z = np.abs(em.binomial_z(counts, N_BIG_SEEDS, N_BIG / (RES * RES))).max()
    print('largest |z|, uniform 128 x 128 map, N = 4096:', z)
    assert z <= Z_BIG


def test_wrong_draws_fail_a_check(big_counts):
    assert _small_z(em.draw_unweighted) > Z_SMALL
    assert _small_z(em.draw_uniform_keys) > Z_SMALL
    z_small = _small_z(em.draw_with_replacement)
    z_big = np.abs(em.binomial_z(big_counts[1], N_BIG_SEEDS, N_BIG / (RES * RES))).max()
    assert z_small > Z_SMALL or z_big > Z_BIG


def test_selection_and_tie_break():
    inf = np.float32(np.inf)
    keys = np.array([inf, 2.0, inf, 0.5, inf, 2.0, inf], np.float32)
    assert em.select(keys, 1).tolist() == [3]
    assert em.select(keys, 2).tolist() == [1, 3]          # equal keys: the lower index
    assert em.select(keys, 3).tolist() == [1, 3, 5]
    assert em.select(keys, 5).tolist() == [0, 1, 2, 3, 5]  # ties among undrawable cells: lowest index first
    assert em.select(keys, 7).tolist() == list(range(7))
    w = np.array([0.0, 1.0, -1.0, np.nan, np.inf, 2.0, 1e-45], np.float32)
    assert em.drawable(w).tolist() == [False, True, False, False, False, True, True]
    k = em.keys64(w, 0, 3)
    assert np.isinf(k[[0, 2, 3, 4]]).all() and np.isfinite(k[[1, 5]]).all() and (k[[1, 5]] > 0).all()
    assert em.draw(w, 5, 0, 3).tolist() == [0, 1, 2, 5, 6]   # the three drawable cells, then undrawable ones from the lowest index


def test_refinement_stays_inside_cell_and_frame():
    for res, H, W in [(128, 800, 800), (33, 37, 101), (8, 1, 1), (3, 5, 2)]:
        cells = np.arange(res * res)
        inds = em.refine(cells, 1, 11, res, H, W)
        row, col = inds // W, inds % W
        assert row.min() >= 0 and row.max() <= H - 1 and col.min() >= 0 and col.max() <= W - 1
        f = np.float32
        lo_r = np.minimum(((cells // res).astype(f) * (f(H) / f(res))).astype(np.int64), H - 1)
        hi_r = np.minimum(np.ceil((cells // res + 1).astype(np.float64) * (f(H) / f(res))).astype(np.int64), H - 1)
        assert np.all(row >= lo_r) and np.all(row <= hi_r)


def test_update_model():
    rng = np.random.default_rng(0)
    row = rng.random(64).astype(np.float32)
    coarse = np.array([3, 70, 9, -1, 63], np.int64)
    img, tgt = rng.random((5, 3)).astype(np.float32), rng.random((5, 3)).astype(np.float32)
    out = em.update(row, coarse, img, tgt)
    touched = np.array([3, 9, 63])
    rest = np.setdiff1d(np.arange(64), touched)
    assert np.array_equal(out[rest].view(np.uint32), row[rest].view(np.uint32))
    want = 0.1 * row[touched].astype(np.float64) + 0.9 * ((img - tgt).astype(np.float64) ** 2).mean(-1)[[0, 2, 4]]
    assert np.allclose(out[touched], want, rtol=1e-6)
