"""CPU: the camera-pose gradient entries at the C ABI -- declared, exported and bound with matching signatures at ABI 11,
refused before any device work on bad arguments, absent from the reference's pybind tables -- the float64 closed forms of
tests/ray_gradient_cases.py against torch autograd of a per-ray loop, and the conditions the GPU tests' inputs must satisfy."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import composite_geo_cases as cg
import grid_forward_cases as gfc
import ray_gradient_cases as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['ngp_ray_sample_ts', 'ngp_ray_sample_ts_f64', 'ngp_ray_points_forward', 'ngp_ray_points_forward_f64', 'ngp_ray_points_backward',
           'ngp_ray_points_backward_f64', 'ngp_grid_input_gradient', 'ngp_rays_from_pixels_backward']


def test_entries_are_declared_exported_and_bound_at_abi_11():
    import _ngp_capi as capi
    header = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_uint32: 'u32', ctypes.c_int: 'int', ctypes.c_float: 'f32'}
    for name in ENTRIES:
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, code, flags=re.S)
        assert m, f'{name} is not declared in include/ngp_hip.h'
        want = []
        for p in m.group(1).split(','):
            p = p.strip()
            want.append('ptr' if '*' in p or p.startswith('ngp_stream_t') else {'uint32_t': 'u32', 'int': 'int', 'float': 'f32'}[p.split()[0]])
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert [kinds[t] for t in fn.argtypes] == want, name
        assert fn.restype is ctypes.c_int
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert f'`{name}`' in table, f'{name} is missing from the INTEGRATION.md table'


def test_the_reference_binding_tables_are_untouched():
    """the entries are ctypes-only: the compiled modules keep the reference's tables"""
    src = open(os.path.join(ROOT, 'torch-ngp_amd', 'csrc', 'bindings.cpp')).read()
    for word in ('ray_sample_ts', 'ray_points', 'grid_input_gradient', 'rays_from_pixels_backward'):
        assert word not in src
    import _raymarching
    import _gridencoder
    for mod in (_raymarching, _gridencoder):
        assert not [n for n in dir(mod) if 'ray_points' in n or 'sample_ts' in n or 'input_gradient' in n]


def _refused(rc, *words):
    import _ngp_capi as capi
    msg = capi.lib.ngp_last_error()
    assert rc == 1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_host_side_refusals_need_no_gpu():
    import _ngp_capi as capi
    lib = capi.lib
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)   # never dereferenced: validation fails first
    # ray_sample_ts
    _refused(lib.ngp_ray_sample_ts(one, one, one, one, 8, 2, 0.0, one, None), 'bound')
    _refused(lib.ngp_ray_sample_ts(one, one, one, one, 8, 2, 1.0, None, None), 'ts', 'NULL')
    _refused(lib.ngp_ray_sample_ts(None, one, one, one, 8, 2, 1.0, one, None), 'xyzs', 'NULL')
    _refused(lib.ngp_ray_sample_ts_f64(one, one, one, one, 8, 2, 1.0, ctypes.c_void_p(68), None), 'ts', 'misaligned')
    assert lib.ngp_ray_sample_ts(None, None, None, None, 0, 4, 1.0, None, None) == 0     # M == 0: nothing to do
    # ray_points_forward
    _refused(lib.ngp_ray_points_forward(one, one, one, one, 8, 2, -1.0, one, one, None), 'bound')
    _refused(lib.ngp_ray_points_forward(one, one, one, one, 8, 2, 1.0, None, one, None), 'xyzs', 'NULL')
    _refused(lib.ngp_ray_points_forward(one, one, one, one, 8, 2, 1.0, one, odd, None), 'dirs', 'misaligned')
    assert lib.ngp_ray_points_forward_f64(None, None, None, None, 0, 0, 1.0, None, None, None) == 0
    # ray_points_backward
    _refused(lib.ngp_ray_points_backward(one, None, None, one, one, one, one, 8, 2, 0.0, one, one, None), 'bound')
    _refused(lib.ngp_ray_points_backward(one, None, None, one, one, one, one, 8, 2, 1.0, None, one, None), 'grad_rays_o', 'NULL')
    _refused(lib.ngp_ray_points_backward(one, None, None, one, one, one, one, 8, 2, 1.0, one, odd, None), 'grad_rays_d', 'misaligned')
    _refused(lib.ngp_ray_points_backward_f64(one, None, one, one, one, one, 8, 2, 1.0, ctypes.c_void_p(68), one, None), 'grad_rays_o', 'misaligned')
    assert lib.ngp_ray_points_backward(None, None, None, None, None, None, None, 8, 0, 1.0, None, None, None) == 0   # N == 0
    # grid_input_gradient: the fused path's layout only
    args = lambda D=3, C=2, L=4, dtype=capi.NGP_F16, g=one, out=one, gridtype=0, interp=0, bound=1.0, M=8: \
        (g, one, one, one, M, D, C, L, 1.0, 4, gridtype, 0, interp, dtype, bound, out, None)
    _refused(lib.ngp_grid_input_gradient(*args(D=2)), 'D = 3, C = 2')
    _refused(lib.ngp_grid_input_gradient(*args(C=4)), 'D = 3, C = 2')
    _refused(lib.ngp_grid_input_gradient(*args(dtype=capi.NGP_F32)), 'float16')
    _refused(lib.ngp_grid_input_gradient(*args(L=0)), 'levels')
    _refused(lib.ngp_grid_input_gradient(*args(L=33)), 'levels')
    _refused(lib.ngp_grid_input_gradient(*args(interp=2)), 'interp')
    _refused(lib.ngp_grid_input_gradient(*args(bound=-1.0)), 'bound')
    _refused(lib.ngp_grid_input_gradient(*args(g=None)), 'grad_enc', 'NULL')
    _refused(lib.ngp_grid_input_gradient(*args(out=odd)), 'grad_xyzs', 'misaligned')
    assert lib.ngp_grid_input_gradient(*args(g=None, out=None, M=0)) == 0
    # rays_from_pixels_backward
    _refused(lib.ngp_rays_from_pixels_backward(one, one, 2, 0.0, 1.0, 0.5, 0.5, 7, None, 0, 4, one, None), 'fx')
    _refused(lib.ngp_rays_from_pixels_backward(one, one, 2, 1.0, 1.0, 0.5, 0.5, 0, None, 0, 4, one, None), 'W')
    _refused(lib.ngp_rays_from_pixels_backward(one, one, 2, 1.0, 1.0, 0.5, 0.5, 7, None, 0, 4, None, None), 'grad_poses', 'NULL')
    _refused(lib.ngp_rays_from_pixels_backward(None, one, 2, 1.0, 1.0, 0.5, 0.5, 7, None, 0, 4, one, None), 'grad_rays_o', 'NULL')
    _refused(lib.ngp_rays_from_pixels_backward(one, one, 2, 1.0, 1.0, 0.5, 0.5, 7, ctypes.c_void_p(68), 0, 4, one, None), 'inds', 'misaligned')
    _refused(lib.ngp_rays_from_pixels_backward(one, one, 1 << 20, 1.0, 1.0, 0.5, 0.5, 7, None, 0, 1 << 20, one, None), '32 bits')
    assert lib.ngp_rays_from_pixels_backward(None, None, 0, 1.0, 1.0, 0.5, 0.5, 7, None, 0, 4, None, None) == 0     # B == 0


def test_python_surface_is_present_and_refuses_without_a_gpu():
    import raymarching
    import nerf.utils
    assert callable(raymarching.sample_ts) and callable(raymarching.ray_points) and callable(nerf.utils.pose_rays)
    import raymarching.raymarching as ops
    assert {'sample_ts', 'ray_points'} <= set(ops.__all__)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        nerf.utils.pose_rays(torch.eye(4)[None], (1.0, 1.0, 0.5, 0.5), 2, 2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            raymarching.ray_points(torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_dir,with_sh', [(False, False), (True, False), (True, True)])
def test_closed_forms_equal_autograd_of_a_per_ray_loop(with_dir, with_sh):
    c = rg.ray_case()
    # a sub-table keeps the O(M) python loop short: every kind of ray up to 'three rows', the planted clamped samples of 'row' included
    rays = c['rays'][:6].copy()
    rays = np.concatenate([rays, c['rays'][-1:]])     # + the overflowing ray
    g_dir = c['g_dir'] if with_dir else None
    g_sh = c['g_sh'] if with_sh else None
    go, gd, S, K = rg.ray_backward_model(c['g_x'], g_dir, g_sh, c['xyzs'], c['ts'], c['rays_d'], rays, rg.RAY_BOUND)
    ao, ad = rg.ray_loop_autograd(c['g_x'], g_dir, g_sh, c['xyzs'], c['ts'], c['rays_o'], c['rays_d'], rays, rg.RAY_BOUND)
    assert np.isfinite(go).all() and np.isfinite(gd).all()
    np.testing.assert_allclose(go, ao, rtol=0, atol=1e-12 * max(1.0, np.abs(ao).max()))
    np.testing.assert_allclose(gd, ad, rtol=0, atol=1e-12 * max(1.0, S.max()))
    empty = [n for n, _, cnt in rays if cnt == 0] + [int(rays[-1, 0])]
    assert (go[empty] == 0).all() and (gd[empty] == 0).all() and K.tolist().count(0) >= len(rays) - 5


def test_ts_model_recovers_the_seeded_ts():
    c = rg.ray_case()
    t = rg.ts_model(c['xyzs'], c['rays_o'], c['rays_d'], c['rays'], rg.RAY_BOUND)
    rows = np.concatenate([np.arange(off, off + cnt) for _, off, cnt in rg.owned(c['rays'], rg.RAY_M)])
    planted = [r for r, _, _ in rg.PLANTED]
    plain = np.setdiff1d(rows, planted)
    # x = fl(o + t d): the quotient recovers t up to the rounding of x, |dx_j| <= 2^-24 |x_j| <= 2^-24 * 2.2, projected on d (|d| = 1)
    clamped = np.any(np.abs(c['xyzs'][plain]) >= rg.RAY_BOUND, axis=1)
    ok = plain[~clamped]
    assert len(ok) > 500
    assert np.abs(t[ok] - c['ts'][ok].astype(np.float64)).max() <= 3 ** 0.5 * 2.2 * rg.U * 4
    assert (t[c['used']:] == 0).all()


def test_pose_model_is_the_stated_closed_form():
    case = rg.pose_case(65, 'per_pose')
    g, S = rg.pose_backward_model(case)
    poses = torch.tensor(case['poses'].astype(np.float64))
    _, _, dcam = rg.rays_from_pixels_torch(poses, rg.POSE_INTRINSICS, rg.POSE_W, case['inds'], case['n'])
    want = np.zeros((rg.POSE_B, 4, 4))
    want[:, :3, 3] = case['grad_o'].astype(np.float64).sum(1)
    want[:, :3, :3] = np.einsum('bnr,bnc->brc', case['grad_d'].astype(np.float64), dcam.numpy())
    np.testing.assert_allclose(g, want, rtol=0, atol=1e-12 * S.max())
    assert (g[:, 3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the GPU tests' inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_ray_case_conditions():
    c1, c2 = rg.ray_case(0), rg.ray_case(1)
    counts = sorted(int(x) for x in c1['rays'][:, 2])
    assert {0, 1, 63, 64, 65, 130, 300} <= set(counts) and rg.RAY_N == 10 and rg.RAY_M == 1600
    assert sum(1 for _, off, cnt in c1['rays'] if off + cnt > rg.RAY_M) == 1
    assert sorted(c1['rays'][:, 0]) == list(range(10)) == sorted(c2['rays'][:, 0]) and c1['rays'][:, 0].tolist() != c2['rays'][:, 0].tolist()
    # every partial sum of grad_rays_o is an integer multiple of 2^-6 below 2^24 units: exact in fp32 in any order
    assert max(counts) * rg.K_MAX < 2 ** 24
    for c in (c1, c2):
        used = c['used']
        for key in ('g_x', 'g_dir'):
            k = c[key][:used].astype(np.float64) * 64
            assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= rg.K_MAX
        k = c['g_sh'][:used].astype(np.float64) * 64
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= rg.K_MAX
        for key in ('xyzs', 'ts', 'g_x', 'g_dir', 'g_sh'):
            assert np.isnan(c[key][used:].astype(np.float64)).all() and np.isfinite(c[key][:used].astype(np.float64)).all()
        for row, j, sign in rg.PLANTED:
            assert c['xyzs'][row, j] == sign * rg.RAY_BOUND and row < used
        assert np.abs(np.linalg.norm(c['rays_d'].astype(np.float64), axis=1) - 1).max() < 1e-6
    # the same rays under both row assignments
    for k in range(rg.RAY_N):
        assert np.array_equal(c1['rays_o'][cg.PERM[k]], c2['rays_o'][rg.PERM2[k]]) and np.array_equal(c1['rays_d'][cg.PERM[k]], c2['rays_d'][rg.PERM2[k]])
    assert np.array_equal(c1['xyzs'][:c1['used']], c2['xyzs'][:c2['used']])


@pytest.mark.parametrize('fc', rg.GRID_EXACT, ids=gfc.case_id)
def test_grid_exact_case_conditions(fc):
    b = fc.base
    assert (b.D, b.C, b.dtype) == (3, 2, 'f16') and b.B == rg.glc.B_SMALL
    out_max, dydx_max, cap = gfc.exact_conditions(fc)
    assert out_max <= cap and dydx_max <= cap          # every dy_dx partial sum is exact (grid_forward_cases)
    ref = rg.grid_exact_reference(fc)
    L = len(b.level_sizes)
    # every product g * dy_dx is a multiple of `unit`, and the sum of their magnitudes stays below 2^24 units: exact in fp32 in any order
    assert L * b.C * rg.G_KMAX * dydx_max < 2 ** 24
    units = ref['want'] / ref['unit']
    assert np.array_equal(units, np.rint(units)) and (ref['absum'] / ref['unit']).max() < 2 ** 24
    assert np.array_equal(ref['want'].astype(np.float32).astype(np.float64), ref['want'])
    k = ref['g'].astype(np.float64) / rg.G_SHIFT
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= rg.G_KMAX
    inside = ref['inside']
    assert (~inside).sum() >= 2 and (ref['want'][~inside] == 0).all() and np.count_nonzero(ref['want'][inside]) > inside.sum()
    if fc.bound > 0.0:
        assert 1.0 / (2.0 * fc.bound) == 0.25
    for B in rg.GRID_EXACT_BS:
        assert len(gfc.point_index(fc, B)) == B
    assert {1, 63, 257} == set(rg.GRID_EXACT_BS)
    # the sweep covers gridtype x align_corners x interpolation
    modes = {(f.base.gridtype, f.base.align, f.base.interp) for f in rg.GRID_EXACT if f.bound == 0.0}
    assert len(modes) == 8 and sum(1 for f in rg.GRID_EXACT if f.bound > 0.0) == 1


@pytest.mark.parametrize('interp,bound', rg.OFF_MODES)
def test_grid_off_lattice_case_conditions(interp, bound):
    c = rg.grid_off_lattice(interp, bound)
    sizes = np.diff(c['offs'])
    assert len(sizes) == 8 and sizes.max() == 2 ** 14 and any(c['dense']) and not all(c['dense'])
    assert c['x'].shape == (1000, 3) and 2 <= (~c['inside']).sum() < 10
    assert (c['want'][~c['inside']] == 0).all() and (np.abs(c['want']) <= c['S_abs'] * (1 + 1e-12)).all()
    assert c['S_abs'][c['inside']].min() > 0


def test_pose_case_conditions():
    for N in rg.POSE_NS:
        for kind in ('shared', 'per_pose', 'none'):
            c = rg.pose_case(N, kind)
            assert c['n'] == (35 if kind == 'none' else N)
            assert np.array_equal(c['grad_o'], np.rint(c['grad_o'])) and c['n'] * 8 < 2 ** 24
            r = c['poses'][:, :3, :3].astype(np.float64)
            assert np.abs(np.einsum('bij,bkj->bik', r, r) - np.eye(3)).max() < 1e-6
