"""raymarching.lattice_points (csrc/surface_nets.hip: k_lattice_count / k_lattice_emit) against the fp32 model of
tests/surface_nets_cases.py, bit for bit: points, index and K.  The model unpacks the bitfield with the Morton helpers of
tests/occupancy_cases.py, dilates the volume and looks every lattice point up in it at the cascade of the marcher's position term."""
import functools

import numpy as np
import pytest
import torch

import occupancy_cases as oc
import surface_nets_cases as sn

pytestmark = pytest.mark.gpu

H = 32                                                    # cells per axis of the occupancy grid: small, so that the lattices straddle cells
LATTICES = [(5, 4, 3), (33, 17, 9), (70, 70, 70)]          # (nx, ny, nz)
FILLS = ('empty', 'full', 'ball', 'random')
CONFIGS = [(1, 1.0, 1.0), (2, 2.0, 2.0), (3, 4.0, 3.7), (2, 2.0, 3.1)]   # (cascades, bound, half-extent of the box): the last box leaves the grid


def _slabs(nz):
    return [(0, nz), (nz // 3, max(nz // 3 + 1, 2 * nz // 3)), (nz - 1, nz)]   # everything, a middle slab, one slice


@functools.lru_cache(maxsize=None)
def _volumes(fill, C):
    """bool [C, z, y, x] occupancy"""
    vol = np.zeros((C, H, H, H), bool)
    if fill == 'full':
        vol[:] = True
    elif fill == 'ball':
        z, y, x = np.meshgrid(*[np.arange(H) + 0.5 - H / 2] * 3, indexing='ij')
        vol[:] = (x - 2.0) ** 2 + (y + 1.0) ** 2 + z ** 2 < (0.3 * H) ** 2
    elif fill == 'random':
        vol[:] = np.random.default_rng(11).random((C, H, H, H)) < 0.1
    return vol


@functools.lru_cache(maxsize=None)
def _dilated(fill, C, dilate):
    return sn.dilate_volumes(_volumes(fill, C), dilate)


@functools.lru_cache(maxsize=None)
def _bits(fill, C):
    bits = oc.pack_volumes(_volumes(fill, C))
    assert np.array_equal(oc.unpack_volumes(bits, C, H), _volumes(fill, C))
    return torch.from_numpy(bits).cuda()


def _check(dims, z0, z1, fill, C, bound, half, dilate):
    import raymarching
    lo, hi = (-half, -0.9 * half, -half), (half, half, 1.1 * half)
    bits = None if fill is None else _bits(fill, C)
    pts, idx = raymarching.lattice_points(lo, hi, dims, z0, z1, bits, bound, C, H, dilate, device='cuda')
    want_p, want_i, keep = sn.lattice_points(lo, hi, dims, z0, z1, bound=bound, cascade=C, grid_size=H, dilate=dilate,
                                             dilated=None if fill is None else _dilated(fill, C, dilate))
    assert pts.dtype == torch.float32 and idx.dtype == torch.int32
    assert pts.shape == want_p.shape and idx.shape == want_i.shape, (pts.shape, want_p.shape)
    assert np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(pts.cpu().numpy().view(np.int32), want_p.view(np.int32))
    return keep


@pytest.mark.parametrize('dims', LATTICES, ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('fill', FILLS)
def test_points_index_and_count_equal_the_model(dims, fill):
    kept = total = 0
    for C, bound, half in CONFIGS:
        for z0, z1 in _slabs(dims[2]):
            for dilate in (0, 1):
                keep = _check(dims, z0, z1, fill, C, bound, half, dilate)
                kept, total = kept + int(keep.sum()), total + keep.size
    assert {'empty': kept == 0, 'full': kept == total}.get(fill, 0 < kept < total)


@pytest.mark.parametrize('dims', LATTICES, ids=lambda d: 'x'.join(map(str, d)))
def test_without_a_bitfield_every_point_is_kept(dims):
    for z0, z1 in _slabs(dims[2]):
        assert _check(dims, z0, z1, None, 1, 1.0, 1.0, 1).all()


def test_dilation_only_adds_points_and_two_runs_agree():
    import raymarching
    dims, args = (70, 70, 70), (_bits('random', 2), 2.0, 2, H)
    a0 = raymarching.lattice_points(-2, 2, dims, 0, 70, *args, 0)
    a1 = raymarching.lattice_points(-2, 2, dims, 0, 70, *args, 1)
    a2 = raymarching.lattice_points(-2, 2, dims, 0, 70, *args, 1)
    assert 0 < len(a0[1]) < len(a1[1]) < 70 ** 3 and torch.isin(a0[1], a1[1]).all()
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])
    assert (a1[1][1:] > a1[1][:-1]).all()                  # lattice order


def test_wrapper_checks_its_arguments():
    import raymarching
    with pytest.raises(RuntimeError, match='slab'):
        raymarching.lattice_points(-1, 1, (4, 4, 4), 2, 2, device='cuda')
    with pytest.raises(RuntimeError, match='slab'):
        raymarching.lattice_points(-1, 1, (4, 4, 4), 0, 5, device='cuda')
    with pytest.raises(RuntimeError, match='bitfield'):
        raymarching.lattice_points(-1, 1, (4, 4, 4), 0, 4, torch.zeros(16, dtype=torch.uint8, device='cuda'), 1, 1, 128)
    with pytest.raises(RuntimeError, match='dilate'):
        raymarching.lattice_points(-1, 1, (4, 4, 4), 0, 4, _bits('ball', 1), 1, 1, H, 5)
