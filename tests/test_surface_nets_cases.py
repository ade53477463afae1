"""The numpy model of the extraction (tests/surface_nets_cases.py) against the properties its definition implies: the GPU
tests compare the kernels with this model, these tests pin the model itself -- closed surfaces, their Euler characteristic, outward
winding (positive signed volume close to the analytic one), both senses of the sign, open surfaces at the box, degenerate shapes; and the
fp32 helpers of the lattice model."""
import math
from fractions import Fraction

import numpy as np
import pytest

import surface_nets_cases as sn


def test_sphere_is_closed_with_euler_2_and_the_analytic_volume():
    v, f = sn.surface_nets(sn.reference_sphere(), 0.0)
    assert len(v) > 2000 and len(f) == 2 * (len(v) - 2)          # Euler characteristic 2 of a closed triangle mesh: F = 2 (V - 2)
    assert sn.is_closed(f) and len(sn.boundary_edges(f)) == 0
    assert sn.euler(len(v), f) == 2
    vol, want = sn.signed_volume(v, f), 4.0 / 3.0 * math.pi * sn.SPHERE_RADIUS ** 3
    print(f'sphere: {len(v)} vertices, {len(f)} triangles, volume {vol / want:.4f} of the analytic value')
    assert vol > 0 and abs(vol / want - 1.0) < 0.02              # positive: the winding points outward
    assert np.abs(np.linalg.norm(v - np.array(sn.SPHERE_CENTRE), axis=1) - sn.SPHERE_RADIUS).max() < math.sqrt(3.0)


def test_torus_is_closed_with_euler_0_and_the_analytic_volume():
    v, f = sn.surface_nets(sn.reference_torus(), 0.0)
    assert sn.is_closed(f) and sn.euler(len(v), f) == 0
    vol, want = sn.signed_volume(v, f), 2.0 * math.pi ** 2 * sn.TORUS_R * sn.TORUS_r ** 2
    print(f'torus: {len(v)} vertices, {len(f)} triangles, volume {vol / want:.4f} of the analytic value')
    assert vol > 0 and abs(vol / want - 1.0) < 0.04


@pytest.mark.parametrize('field', ['sphere', 'noise'])
def test_inside_below_of_the_negated_volume_is_the_same_mesh(field):
    f = sn.reference_sphere() if field == 'sphere' else sn.noise((9, 10, 11))
    level = 0.0 if field == 'sphere' else 0.5
    v0, f0 = sn.surface_nets(f, level)
    v1, f1 = sn.surface_nets(-f, -level, inside_below=True)
    assert np.array_equal(f0, f1) and np.array_equal(v0, v1)


def test_noise_never_repeats_a_vertex_in_a_triangle():
    v, f = sn.surface_nets(sn.noise((17, 18, 19)), 0.5)
    assert len(f) > 1000 and f.min() >= 0 and f.max() < len(v)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    # one vertex per cell that a crossing edge touches: every vertex of an interior cell is used
    assert len(np.unique(f)) <= len(v)


def test_a_sphere_cut_by_the_box_is_open_and_emits_nothing_on_boundary_edges():
    shape = (20, 20, 20)
    f = sn.sphere(shape, 6.3, (3.37, 9.61, 9.43))                # leaves the box through the face x = 0 only
    v, faces = sn.surface_nets(f, 0.0)
    assert len(faces) > 0 and not sn.is_closed(faces)
    rim = sn.boundary_edges(faces)
    assert len(rim) > 0
    # the rim's vertices belong to the cells of the first layer at x = 0 (cells whose boundary edges were skipped)
    assert v[np.unique(rim), 0].max() < 1.0
    # nothing is emitted for a boundary edge: the count equals two triangles per INTERIOR crossing edge
    inside = f > 0
    nz, ny, nx = shape
    n = (inside[1:-1, 1:-1, :-1] != inside[1:-1, 1:-1, 1:]).sum() + (inside[1:-1, :-1, 1:-1] != inside[1:-1, 1:, 1:-1]).sum() + \
        (inside[:-1, 1:-1, 1:-1] != inside[1:, 1:-1, 1:-1]).sum()
    assert len(faces) == 2 * n


@pytest.mark.parametrize('shape,has_faces', [((2, 2, 2), False), ((2, 5, 4), True), ((3, 3, 3), True)])
def test_smallest_shapes(shape, has_faces):
    """(2,2,2) has no interior edge: vertices, zero faces.  (2,5,4) -- two lattice planes -- has no interior x- or y-edge (1 <= p_z <= nz - 2 is
    empty), so a surface between its columns emits vertices and no faces; its z-edges at 1 <= p_x <= 2, 1 <= p_y <= 3 ARE interior by the
    definition and emit a sheet between the planes."""
    f = sn.noise(shape, seed=3)
    if shape == (3, 3, 3):
        f[1, 1, 1], f[1, 1, 2] = 2.0, -2.0                        # the one interior x-edge crosses
    if shape == (2, 5, 4):
        columns = np.where(np.arange(4) < 2, 2.0, -2.0).astype(np.float32) * np.ones(shape, np.float32)   # changes along x only
        v, faces = sn.surface_nets(columns, 0.5)
        assert len(v) == 4 and len(faces) == 0
        f[0], f[1] = 2.0, -2.0                                    # changes along z only: six interior z-edges
        assert len(sn.surface_nets(f, 0.5)[1]) == 12
    v, faces = sn.surface_nets(f, 0.5)
    assert len(v) > 0 and v.shape[1] == 3 and faces.shape[1:] == (3,) and faces.dtype == np.int32
    assert (len(faces) > 0) == has_faces
    cells = np.array(shape[::-1]) - 1
    assert (v >= 0).all() and (v <= cells).all()


def test_ties_nan_and_infinities_count_as_stated():
    f = np.full((3, 3, 3), -1.0, np.float32)
    f[1, 1, 1] = 0.0                                              # s == 0: outside -> nothing
    assert len(sn.surface_nets(f, 0.0)[0]) == 0
    f[1, 1, 1] = np.nan
    assert len(sn.surface_nets(f, 0.0)[0]) == 0
    f[1, 1, 1] = np.inf                                           # inside: a closed cell-sized box around the point
    v, faces = sn.surface_nets(f, 0.0)
    assert len(v) == 8 and len(faces) == 12 and sn.is_closed(faces) and sn.signed_volume(v, faces) > 0
    # seen from the outside corner a the crossing is t = -1 / (-1 - inf) = 0, from the inside corner inf / (inf + 1) = NaN -> 0.5
    assert np.allclose(np.unique(v.round(12)), [2.0 / 3.0, 1.0 + 0.5 / 3.0])
    assert len(sn.surface_nets(np.ones((4, 4, 4), np.float32), 0.0)[0]) == 0   # all inside
    origin, spacing = (-1.0, 2.0, 0.5), (0.5, 0.25, 2.0)
    w, _ = sn.surface_nets(f, 0.0, origin=origin, spacing=spacing)
    assert np.allclose(w, v * np.array(spacing) + np.array(origin))


def test_position_tolerance_is_a_few_ulps_of_the_extent():
    tol = sn.position_tolerance((129, 129, 129), (-1.0, -1.0, -1.0), (2.0 / 128,) * 3)
    assert (tol > 2.0 ** -24 * 2.0).all() and (tol < 2.0 ** -24 * 8.0).all()


def test_fma32_rounds_once():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 20, 4000).astype(np.float32)
    b = (rng.standard_normal(4000) * 0.01).astype(np.float32)
    c = rng.standard_normal(4000).astype(np.float32)
    # a tie of the float64 sum that a double rounding gets wrong: 2^24 + 1 + 2^-30 is above the midpoint of 2^24 and 2^24 + 2
    a[0], b[0], c[0] = np.float32(2.0 ** 24 + 2) / 2, 2.0, np.float32(-1.0)
    a[1], b[1], c[1] = np.float32(2.0 ** -30), 1.0, np.float32(2.0 ** 24)
    a[2], b[2], c[2] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** 30)
    got = sn.fma32(a, b, c)
    # the exact value in rationals, rounded ONCE: the nearest of the fp32 neighbours of a first guess, ties to the even mantissa
    exact = []
    for x, y, z in zip(a, b, c):
        q = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        guess = np.float32(float(q))
        cands = [guess, np.nextafter(guess, np.float32(np.inf)), np.nextafter(guess, np.float32(-np.inf))]
        exact.append(min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.float32(v).view(np.uint32)) & 1)))
    assert np.array_equal(got, np.array(exact, np.float32))


def test_lattice_model_keeps_everything_without_a_bitfield_and_orders_by_index():
    pts, idx, keep = sn.lattice_points((-1, -1, -1), (1, 1, 1), (5, 4, 3), 1, 3)
    assert keep.all() and len(pts) == 5 * 4 * 2 and np.array_equal(idx, np.arange(20, 60, dtype=np.int32))
    assert np.array_equal(pts[0], np.array([-1.0, -1.0, 0.0], np.float32)) and np.array_equal(pts[-1], np.array([1.0, 1.0, 1.0], np.float32))


def test_lattice_cells_follow_the_cascades():
    x = np.array([0.3, 0.99, 1.0, 1.7, -3.9, 5.0], np.float32)
    zero = np.zeros_like(x)
    level, cx, cy, cz = sn.lattice_cells(x, zero, zero, 4.0, 3, 128)
    assert level.tolist() == [0, 0, 1, 1, 2, 2]                   # frexp exponent of max |x|, clamped to the cascades
    assert cx.tolist() == [83, 127, 96, 118, 1, 127] and (cy == 64).all() and (cz == 64).all()
