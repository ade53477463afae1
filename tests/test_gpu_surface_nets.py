"""raymarching.surface_nets (csrc/surface_nets.hip) against the numpy model of tests/surface_nets_cases.py.

Faces and the order of the vertices are compared exactly: the topology is decided by the fp32 sign s = f - level, which kernel and model
compute with the same correctly rounded subtraction.  Positions are compared with the float64 model under the bound of
surface_nets_cases.position_tolerance, derived from the kernel's arithmetic (u = 2^-24): t = s_a / (s_a - s_b) -> 2 u; the sum of n <= 12 terms
in [0, 1] -> n (n + 1) / 2 u; the division -> 9.5 u on the mean; the integer cell coordinate -> N u; one fma -> (N h + |o|) u: in total
u (2 N h + 10 h + |o|), a few ulps of max(N h, |o|).  Worst error seen on an MI355X: see WORST_SEEN below (as a fraction of that bound)."""
import functools

import numpy as np
import pytest
import torch

import surface_nets_cases as sn

pytestmark = pytest.mark.gpu

# the largest |kernel - model| / bound over every case of test_mesh_equals_the_model (printed by the test; MI355X, ROCm 7.2)
WORST_SEEN = 0.76

SHAPES = [(2, 2, 2), (3, 3, 3), (3, 4, 5), (9, 9, 9), (17, 9, 33), (5, 3, 130), (70, 70, 70), (129, 129, 129)]   # (nz, ny, nx)
FIELDS = ('sphere', 'torus', 'noise', 'plane', 'specials', 'all inside', 'all outside')
ORIGIN, SPACING = (-1.25, 0.5, 3.0), (0.03125, 0.0123, 0.25)


def _field(name, shape):
    """-> (volume, level) with inside above the level"""
    if name == 'sphere':
        return sn.fitted_sphere(shape), 0.0
    if name == 'torus':
        return sn.fitted_torus(shape), 0.0
    if name == 'noise':
        return sn.noise(shape), 0.5
    if name == 'plane':
        return sn.plane_on_lattice(shape), 0.0
    if name == 'specials':
        return sn.noise_with_specials(shape), 0.5
    return np.full(shape, 1.0 if name == 'all inside' else -1.0, np.float32), 0.0


@functools.lru_cache(maxsize=None)
def _reference(name, shape, below):
    """-> (volume, level, inside_below, vertices, faces): every model result is computed once and shared (read-only)"""
    f, level = _field(name, shape)
    vol, lv = (-f, -level) if below else (f, level)
    return (vol, lv, below) + sn.surface_nets(vol, lv, below, ORIGIN, SPACING)


def _senses(shape):
    """both senses of inside_below on every shape but the largest, whose model runs take a second each"""
    return (False,) if shape == (129, 129, 129) else (False, True)


def _run(vol, level, below, origin=ORIGIN, spacing=SPACING):
    import raymarching
    v, f = raymarching.surface_nets(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), level, below, origin, spacing)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v.cpu().numpy(), f.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_mesh_equals_the_model(shape):
    worst = 0.0
    tol = sn.position_tolerance(shape, ORIGIN, SPACING)
    for name, below in [(n, b) for n in FIELDS for b in _senses(shape)]:
        vol, level, _, want_v, want_f = _reference(name, shape, below)
        got_v, got_f = _run(vol, level, below)
        assert got_v.shape == want_v.shape and got_f.shape == want_f.shape, (name, below, got_v.shape, want_v.shape, got_f.shape, want_f.shape)
        assert np.array_equal(got_f, want_f), (name, below)
        if name.startswith('all'):
            assert len(got_v) == 0 and len(got_f) == 0
        if len(got_v) == 0:
            continue
        err = np.abs(got_v.astype(np.float64) - want_v) / tol
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (name, below, float(err.max()))
    print(f'{shape}: worst position error {worst:.3f} of the bound')


def test_both_senses_give_the_same_mesh():
    for name in ('sphere', 'noise', 'specials'):
        a, b = _reference(name, (9, 9, 9), False), _reference(name, (9, 9, 9), True)
        got_a, got_b = _run(*a[:3]), _run(*b[:3])
        # NaN stays outside in both senses, so the negated volume with specials differs only where the model says so
        assert np.array_equal(got_a[1], a[4]) and np.array_equal(got_b[1], b[4])
        if name != 'specials':
            assert np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[1], got_b[1])


def test_default_frame_is_the_lattice():
    vol, level, below, _, want_f = _reference('torus', (17, 9, 33), False)
    want_v, _ = sn.surface_nets(vol, level, below)
    got_v, got_f = _run(vol, level, below, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert np.array_equal(got_f, want_f)
    assert (np.abs(got_v - want_v) <= sn.position_tolerance((17, 9, 33), (0, 0, 0), (1, 1, 1))).all()
    assert got_v.min() >= 0 and (got_v.max(axis=0) <= np.array([32, 8, 16])).all()


def test_two_runs_give_the_same_bits():
    for key in (('noise', (70, 70, 70), False), ('specials', (17, 9, 33), True)):
        vol, level, below = _reference(*key)[:3]
        a, b = _run(vol, level, below), _run(vol, level, below)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_emit_with_short_buffers_truncates_and_reports():
    """capacities one below the counts: the error, the rows that fit as in the full mesh, and the guard rows behind the buffers untouched"""
    from raymarching import backend
    vol, level, below, want_v, want_f = _reference('noise', (9, 9, 9), False)
    n_v, n_f = len(want_v), len(want_f)
    dev = torch.device('cuda')
    volume = torch.from_numpy(vol).to(dev)
    ws = backend.surface_nets_workspace(volume)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    backend.surface_nets_count(volume, level, below, ws, counts)
    assert counts.tolist() == [n_v, n_f]
    guard = 7
    vbuf = torch.full((n_v - 1 + guard, 3), -77.0, device=dev)
    fbuf = torch.full((n_f - 1 + guard, 3), -77, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match='truncated'):
        backend.surface_nets_emit(volume, level, below, ORIGIN, SPACING, ws, vbuf[:n_v - 1], fbuf[:n_f - 1])
    torch.cuda.synchronize()
    assert (vbuf[n_v - 1:] == -77.0).all() and (fbuf[n_f - 1:] == -77).all()
    full_v, full_f = _run(vol, level, below)
    assert np.array_equal(vbuf[:n_v - 1].cpu().numpy(), full_v[:-1]) and np.array_equal(fbuf[:n_f - 1].cpu().numpy(), full_f[:-1])
    # exact capacities: no error
    vbuf, fbuf = torch.empty(n_v, 3, device=dev), torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    backend.surface_nets_emit(volume, level, below, ORIGIN, SPACING, ws, vbuf, fbuf)
    assert np.array_equal(fbuf.cpu().numpy(), want_f)


def test_wrapper_checks_its_arguments():
    import raymarching
    with pytest.raises(RuntimeError, match=r'\[nz, ny, nx\]'):
        raymarching.surface_nets(torch.zeros(4, 4, device='cuda'), 0.0)
    with pytest.raises(RuntimeError, match='at least 2'):
        raymarching.surface_nets(torch.zeros(4, 1, 4, device='cuda'), 0.0)
    with pytest.raises(RuntimeError, match='float32'):
        raymarching.surface_nets(torch.zeros(4, 4, 4, device='cuda', dtype=torch.float64), 0.0)
    v, f = raymarching.surface_nets(torch.zeros(4, 4, 4, device='cuda'), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32
