"""NeRFRenderer.extract_mesh and NeuSNetwork.extract_mesh end to end: the culled fill of the volume, the extraction, the
mesh's properties.  The mesh is compared with the numpy model applied to the volume the call returns, so the tests do not depend on how the
GPU rounds the field."""
import math

import numpy as np
import pytest
import torch

import occupancy_cases as oc
import surface_nets_cases as sn

pytestmark = pytest.mark.gpu

RADIUS, CENTRE, SHARPNESS = 0.53, (0.11, -0.07, 0.05), 60.0
RES = 96


def _ball_model(cuda_ray=True):
    from nerf.renderer import NeRFRenderer

    class Ball(NeRFRenderer):
        """an analytic density: a sharp ball, 20 inside, 0 outside, the default level 10 exactly at RADIUS"""

        def density(self, x):
            c = torch.tensor(CENTRE, dtype=torch.float32, device=x.device)
            r = torch.sqrt(((x.float() - c) ** 2).sum(-1))
            return {'sigma': 20.0 * torch.sigmoid(SHARPNESS * (RADIUS - r))}

    m = Ball(bound=1, cuda_ray=cuda_ray).cuda()
    if cuda_ray:
        # the bitfield: the cells of the 128^3 grid within two cells of the ball
        H = m.grid_size
        z, y, x = np.meshgrid(*[(np.arange(H) + 0.5) / H * 2 - 1] * 3, indexing='ij')
        r = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)
        vol = (r < RADIUS + 2 * (2.0 / H))[None]
        m.density_bitfield.copy_(torch.from_numpy(oc.pack_volumes(vol)).cuda())
        m._occupancy = vol
    return m


@pytest.fixture(scope='module')
def ball():
    m = _ball_model()
    v, f, volume = m.extract_mesh(resolution=RES, cull=False, return_volume=True)
    torch.cuda.synchronize()
    return m, v.cpu().numpy(), f.cpu().numpy(), volume.cpu().numpy()


def _against_model(v, f, volume, level, below, lo, hi, dims):
    o, h = sn.lattice_spacing(lo, hi, dims)
    want_v, want_f = sn.surface_nets(volume, level, below, o, h)
    assert np.array_equal(f, want_f) and v.shape == want_v.shape
    assert (np.abs(v - want_v) <= sn.position_tolerance(volume.shape, o, h)).all()


def test_dense_fill_equals_the_model_on_the_returned_volume(ball):
    m, v, f, volume = ball
    assert volume.shape == (RES, RES, RES) and volume.dtype == np.float32
    _against_model(v, f, volume, 10.0, False, (-1,) * 3, (1,) * 3, (RES,) * 3)
    # the volume IS the field on the lattice: 20 deep inside, 0 far outside
    assert volume.max() > 19.9 and volume.min() < 1e-6


def test_the_ball_is_closed_round_and_of_the_right_volume(ball):
    m, v, f, volume = ball
    h = 2.0 / (RES - 1)
    assert len(f) > 0 and sn.is_closed(f) and sn.euler(len(v), f) == 2
    dist = np.abs(np.linalg.norm(v - np.array(CENTRE), axis=1) - RADIUS)
    assert dist.max() < math.sqrt(3.0) * h, dist.max()
    vol, want = sn.signed_volume(v, f), 4.0 / 3.0 * math.pi * RADIUS ** 3
    assert vol > 0 and abs(vol / want - 1.0) < 0.02, vol / want   # the margin of tests/test_surface_nets_cases.py's sphere


def test_culled_fill_gives_the_same_bits_and_evaluates_less(ball):
    import raymarching
    m, v, f, volume = ball
    cv, cf, cvol = m.extract_mesh(resolution=RES, cull=True, return_volume=True)
    assert np.array_equal(cv.cpu().numpy().view(np.int32), v.view(np.int32)) and np.array_equal(cf.cpu().numpy(), f)
    # the kept-point mask, from the same call extract_mesh makes
    _, index = raymarching.lattice_points(-1, 1, (RES,) * 3, 0, RES, m.density_bitfield, m.bound, m.cascade, m.grid_size, 1)
    keep = np.zeros(RES ** 3, bool)
    keep[index.cpu().numpy()] = True
    keep = keep.reshape(RES, RES, RES)
    assert 0.0 < keep.mean() < 1.0
    print(f'kept {keep.mean():.4f} of the lattice points')
    # ... equals the model's mask, and the culled volume is the dense one on it and the fill elsewhere
    _, _, want_keep = sn.lattice_points((-1,) * 3, (1,) * 3, (RES,) * 3, 0, RES, bound=1.0, cascade=1, grid_size=m.grid_size, dilate=1,
                                        dilated=sn.dilate_volumes(m._occupancy, 1))
    assert np.array_equal(keep, want_keep)
    cvol = cvol.cpu().numpy()
    assert np.array_equal(cvol[keep], volume[keep]) and (cvol[~keep] == 0.0).all()
    # every endpoint of a crossing edge lies inside the dilated occupancy
    inside = volume > 10.0
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        cross = inside[tuple(a)] != inside[tuple(b)]
        assert cross.any() and keep[tuple(a)][cross].all() and keep[tuple(b)][cross].all()


def test_three_slabs_give_the_same_mesh_as_one(ball):
    m, v, f, volume = ball
    sv, sf, svol = m.extract_mesh(resolution=RES, cull=True, slab_points=RES * RES * (RES // 3 + 1), return_volume=True)
    assert np.array_equal(sv.cpu().numpy().view(np.int32), v.view(np.int32)) and np.array_equal(sf.cpu().numpy(), f)
    dv, df = m.extract_mesh(resolution=RES, cull=False, slab_points=RES * RES * (RES // 3 + 1))
    assert np.array_equal(dv.cpu().numpy().view(np.int32), v.view(np.int32)) and np.array_equal(df.cpu().numpy(), f)


def test_resolution_triple_and_box(ball):
    m = ball[0]
    dims, lo, hi = (40, 33, 50), (-0.8, -0.9, -0.75), (0.9, 0.8, 0.85)
    v, f, volume = m.extract_mesh(resolution=dims, lo=lo, hi=hi, cull=True, return_volume=True)
    assert tuple(volume.shape) == (50, 33, 40)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    _against_model(v, f, volume.cpu().numpy(), 10.0, False, lo, hi, dims)
    assert sn.is_closed(f) and sn.euler(len(v), f) == 2


def test_cull_needs_cuda_ray():
    m = _ball_model(cuda_ray=False)
    with pytest.raises(RuntimeError, match='cuda_ray'):
        m.extract_mesh(resolution=16)
    v, f = m.extract_mesh(resolution=32, cull=False)
    assert len(v) > 0 and sn.is_closed(f.cpu().numpy())


def test_neus_network_at_initialisation():
    """the sphere prior gives a surface before any training: |x| = prior_radius up to what the untrained network adds"""
    from nerf.network_sdf import NeuSNetwork
    torch.manual_seed(0)
    m = NeuSNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, prior_radius=0.5).cuda()
    was_training = m.training
    v, f, volume, n = m.extract_mesh(resolution=64, cull=False, return_volume=True, normals=True)
    assert m.training == was_training
    v, f, volume, n = v.cpu().numpy(), f.cpu().numpy(), volume.cpu().numpy(), n.cpu().numpy()
    assert len(v) > 0 and len(f) > 0 and sn.is_closed(f)
    _against_model(v, f, volume, 0.0, True, (-1,) * 3, (1,) * 3, (64,) * 3)
    assert n.shape == v.shape and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-4
    assert sn.signed_volume(v, f) > 0                                      # inside is below the level: the winding still points outward
    assert (np.einsum('ij,ij->i', n, v) > 0).mean() > 0.99                 # ... and so does the SDF's gradient
    # the bitfield of a fresh model is empty: a culled fill evaluates nothing and leaves the fill (+1: outside) -> an empty mesh
    ev, ef = m.extract_mesh(resolution=32)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    # with the occupancy refreshed from the model's own density the culled mesh is the dense one
    with torch.autocast('cuda', dtype=torch.float16):
        m.update_extra_state()
    cv, cf = m.extract_mesh(resolution=64, cull=True)
    assert np.array_equal(cf.cpu().numpy(), f) and np.array_equal(cv.cpu().numpy().view(np.int32), v.view(np.int32))


def test_save_mesh_writes_what_extract_mesh_returns(ball, tmp_path):
    from nerf.utils import save_mesh
    m, v, f, volume = ball
    path = str(tmp_path / 'ball.ply')
    save_mesh(path, torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + 11
    assert f'element vertex {len(v)}'.encode() in raw[:end] and f'element face {len(f)}'.encode() in raw[:end]
    assert np.array_equal(np.frombuffer(raw, '<f4', 3 * len(v), end).reshape(-1, 3), v)
    assert len(raw) == end + 12 * len(v) + 13 * len(f)
