"""CPU checks of the shared cases of tests/sdf_sigmas_cases.py themselves (raymarching.sdf_sigmas): the sample table meets
the conditions its comparisons rely on, the cancellation-free definition IS NeuS's opacity, and its densities composite to NeuS's weights."""
import math

import numpy as np
import torch

import composite_geo_cases as G
import sdf_sigmas_cases as C


def test_sample_table_meets_its_conditions():
    t = C.sample_table()
    d0 = t['deltas'][:, 0]
    assert C.M == 1600 and C.LIVE == 1500 and (d0[C.LIVE:] == 0).all() and (d0[:C.LIVE] >= 0.005 - 1e-9).all() and (d0[:C.LIVE] <= 0.05 + 1e-9).all()
    for k in ('sdf', 'normals', 'dirs', 'deltas', 'up'):
        assert np.isfinite(t[k]).all() and np.array_equal(t[k], t[k].astype(np.float32).astype(np.float64)), k   # float32-representable
    live = slice(0, C.LIVE)
    assert np.abs(t['sdf'][live]).max() <= 0.1 + 1e-8
    norm = np.linalg.norm(t['normals'][live], axis=1)
    assert norm.min() >= 0.7 - 1e-6 and norm.max() <= 1.3 + 1e-6
    assert np.abs(np.linalg.norm(t['dirs'][live], axis=1) - 1.0).max() < 1e-6
    assert (t['up'][C.LIVE:] != 0).all()                         # the padding rows carry an upstream gradient: zeros there are the op's doing
    c = (t['dirs'][live] * t['normals'][live]).sum(1)
    assert np.abs(c).min() >= C.KINK and np.abs(c - 1.0).min() >= C.KINK   # no row on a relu kink of the cosine
    assert (c < 0).any() and (c > 0).any() and (c > 1).any()      # every branch of the cosine
    for inv_s, ca in C.GRID:
        ref = C.reference(inv_s, ca)
        assert np.abs(ref['x_raw'][live] - C.X_MAX).min() >= C.CAP_MARGIN, (inv_s, ca)
        frac = ref['capped'][live].mean()
        assert (frac >= 0.2) if inv_s >= 512 else (frac == 0.0), (inv_s, ca, frac)
        assert not ref['capped'][C.LIVE:].any()
        # what the reference says about the rows the kernels treat specially
        assert (ref['sigma'][C.LIVE:] == 0).all() and (ref['grad_sdf'][C.LIVE:] == 0).all() and (ref['grad_normals'][C.LIVE:] == 0).all()
        cap = ref['capped']
        assert (ref['grad_sdf'][cap] == 0).all() and (ref['grad_normals'][cap] == 0).all() and (ref['grad_dirs'][cap] == 0).all()
        assert (ref['grad_sdf'][live][~cap[live]] != 0).all()


def test_definition_is_the_literal_neus_opacity():
    t = C.sample_table()
    a = lambda k: torch.from_numpy(t[k][:C.LIVE])
    for inv_s, ca in C.GRID:
        ref = C.reference(inv_s, ca)
        lit = C.literal_alpha(a('sdf'), a('normals'), a('dirs'), a('deltas')[:, 0], torch.tensor(inv_s, dtype=torch.float64), ca).numpy()
        got = -np.expm1(-ref['x'][:C.LIVE])
        cap = ref['capped'][:C.LIVE]
        assert np.abs(got - lit)[~cap].max() <= 1e-13, (inv_s, ca)
        if cap.any():
            assert np.abs(got - lit)[cap].max() <= math.exp(-C.X_MAX) + 1e-12, (inv_s, ca)
        assert ((lit > 0) & (lit <= 1)).all()                      # (h <= 0: the clip of the literal formula is never active from below)


def test_reference_densities_composite_to_the_neus_weights():
    """sigma_ref through the float64 definition of the compositor (composite_geo_cases.reference) against NeuS's rendering with literal alphas
    on that module's ray layout"""
    r, lit = C.ray_case(), C.ray_literal()
    assert lit['min_T'] > 5 * G.T_THRESH                            # no ray ends early: no sample on the T_thresh discontinuity
    sig = C.ray_sigmas(torch.float64)
    assert (sig * r['deltas'][:, 0]).max() < C.X_MAX - 1.0          # no capped row here: the agreement below is to rounding
    got = G.reference(sig, r['rgbs'], r['deltas'], r['rays'])
    counts = [int(n) if o + n <= len(sig) else 0 for _, o, n in r['rays']]
    assert got['live'] == counts
    for key in ('weights_sum', 'depth', 'image'):
        assert np.abs(got[key] - lit[key]).max() <= 1e-13, key
    assert lit['weights_sum'].max() > 0.8 and (lit['weights_sum'] == 0).sum() == 2   # the empty and the overflowing ray
    for key in ('weights_sum', 'depth', 'image'):
        bound, err = C.ray_yardstick(key)
        assert 0 < err < 1e-4 and bound < 1e-3, key


def test_yardsticks_are_rounding_sized():
    for key in C.KEYS:
        bound, err = C.yardstick(key)
        ref_max = max(float(np.abs(C.reference(*g)[key]).max()) for g in C.GRID)
        assert 0 < err and bound < 1e-4 * max(ref_max, 1.0), (key, bound, err, ref_max)
