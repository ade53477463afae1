"""The atomic grid backward (k_grid_backward / backward_atomic_block / corner_runs in csrc/gridencoder.hip) and the atomic workgroups that
ride in the record-sort launch (the AtomicPart branch of k_grid_backward_bin), bit for bit against the float64 oracle.

(a)-(d) run on lattice inputs whose sums have no rounding (tests/grid_lattice_cases.py; the conditions on those inputs are asserted on the
CPU by tests/test_grid_lattice_cases.py): a lost, doubled or misrouted contribution changes the bits.  (e) runs ray-ordered samples off the
lattice against a per-entry bound made from the oracle alone, (f) grad_total_variation over its template / argument space."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import grid_lattice_cases as glc

pytestmark = pytest.mark.gpu

TORCH = {'f16': torch.float16, 'f32': torch.float32}
NUMPY = {'f16': np.float16, 'f32': np.float32}
BITS = {'f16': torch.int16, 'f32': torch.int32}


def _capi():
    import _ngp_capi as capi
    return capi


def _code(dtype):
    return _capi().NGP_F16 if dtype == 'f16' else _capi().NGP_F32


def _host(offs):
    return (ctypes.c_int32 * len(offs))(*[int(v) for v in offs])


def _backward(x, g, offs, S, H, dtype, gridtype=0, align=False, interp=0, prefill=0.0, use_workspace=False, bound=0.0):
    """ngp_grid_encode_backward_ws over D, C, dtype and the index modes.  workspace = NULL: the atomic kernel is certain to run.
    Returns the gradient table (on the host) and the workspace size the plan asked for."""
    capi = _capi()
    L, B, C = g.shape
    D = x.shape[1]
    gt = torch.tensor(g).cuda().to(TORCH[dtype])   # (copies: the cached case arrays are read-only)
    xt = torch.tensor(x).cuda()
    ot = torch.tensor(offs).cuda()
    ge = torch.full((int(offs[-1]), C), prefill, device='cuda', dtype=TORCH[dtype])
    arr = _host(offs)
    nbytes, ws = 0, None
    if use_workspace:
        nbytes = int(capi.lib.ngp_grid_backward_workspace_bytes(ctypes.cast(arr, ctypes.c_void_p), B, D, C, L, S, H, gridtype, int(align), _code(dtype)))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device='cuda').fill_(0xAB)   # contents irrelevant
    capi.check(capi.lib.ngp_grid_encode_backward_ws(gt.data_ptr(), xt.data_ptr(), None, ot.data_ptr(), ge.data_ptr(), B, D, C, L, S, H, None, None,
                                                    gridtype, int(align), interp, _code(dtype), bound,
                                                    ctypes.cast(arr, ctypes.c_void_p) if use_workspace else None,
                                                    capi.ptr(ws) if use_workspace and nbytes else None, nbytes, capi.stream()))
    torch.cuda.synchronize()
    return ge.cpu(), nbytes


def _assert_bits(got, want64, case, what):
    """got (a tensor of the table type) has exactly the bits of the float64 reference cast to the table type"""
    want = torch.from_numpy(want64.astype(NUMPY[case.dtype]))
    assert np.array_equal(want.double().numpy(), want64), 'the reference is representable in the table type'
    if torch.equal(got.view(BITS[case.dtype]), want.view(BITS[case.dtype])):
        return
    diff = (got.double() - want.double()).numpy() / glc.unit_of(case)
    bad = np.argwhere(diff != 0)
    lines = ['entry %d channel %d: off by %g units (reference %g units)' % (e, c, diff[e, c], want64[e, c] / glc.unit_of(case)) for e, c in bad[:8]]
    raise AssertionError('%s, %s: %d of %d values differ from the exact sum\n  %s' % (glc.case_id(case), what, len(bad), diff.size, '\n  '.join(lines)))


def _check_exact(case, x=None, **kw):
    """both runs of a case: into a zeroed table and into one pre-filled with 0.25 (+=)"""
    xs, g, offs, S = glc.make(case)
    e = glc.exactness(case)
    assert (glc.PREFILL + e['A'].max()) / e['unit'] < e['cap'] and e['runs'].max() >= 100
    out = []
    for prefill in (0.0, glc.PREFILL):
        got, nbytes = _backward(xs if x is None else x, g, offs, S, case.H, case.dtype, case.gridtype, case.align, case.interp, prefill=prefill, **kw)
        _assert_bits(got, prefill + e['ref'], case, 'table pre-filled with %g' % prefill)
        out.append((got, nbytes))
    return out


# (a) every lane layout: 2 dtypes x C in {1, 2, 4, 8} x D in {2, 3, 4, 5}, the index modes in rotation
@pytest.mark.parametrize('case', glc.LAYOUT_CASES, ids=glc.case_id)
def test_every_lane_layout_is_exact(case):
    _check_exact(case)


# (b) gridtype x align_corners x interpolation, three levels of three sizes (per-level offsets, sizes, LevelList)
@pytest.mark.parametrize('case', glc.SWEEP_CASES, ids=glc.case_id)
def test_every_index_mode_is_exact_over_three_levels(case):
    _check_exact(case)


# (c) the in-kernel input mapping: world coordinates 4 x - 2 at bound = 2, the oracle on the unit lattice
@pytest.mark.parametrize('case', glc.MAPPED_CASES, ids=glc.case_id)
def test_input_mapping_is_exact(case):
    capi = _capi()
    x, g, offs, S = glc.make(case)
    xw = glc.world_coordinates(x)
    _check_exact(case, x=xw, bound=glc.BOUND)
    # and through the entry point the module calls
    L, B, C = g.shape
    ge = torch.zeros(int(offs[-1]), C, device='cuda', dtype=TORCH[case.dtype])
    gt = torch.tensor(g).cuda().to(TORCH[case.dtype])
    xt = torch.tensor(xw).cuda()
    ot = torch.tensor(offs).cuda()
    capi.check(capi.lib.ngp_grid_encode_backward_ex(gt.data_ptr(), xt.data_ptr(), None, ot.data_ptr(), ge.data_ptr(), B, case.D, C, L, S, case.H, None, None,
                                                    case.gridtype, int(case.align), case.interp, _code(case.dtype), glc.BOUND, capi.stream()))
    torch.cuda.synchronize()
    _assert_bits(ge.cpu(), glc.exactness(case)['ref'], case, 'ngp_grid_encode_backward_ex')


# (d) atomic levels riding in the record-sort launch: backward_atomic_block<half, D, 2, 3, BIN_THREADS>, 512 threads, 1024 points per
# workgroup, its own block -> level mapping.  One level is binned and one is not (glc.SORT_LAUNCH_CASES says which branch of
# plan_backward refuses it), in both orders.
@pytest.mark.parametrize('case', glc.SORT_LAUNCH_CASES, ids=glc.case_id)
def test_atomic_levels_in_the_sort_launch_are_exact(case):
    capi = _capi()
    _, g, offs, S = glc.make(case)
    L, B, C = g.shape
    arr = ctypes.cast(_host(offs), ctypes.c_void_p)
    args = (B, case.D, C, L, S, case.H, case.gridtype, int(case.align), capi.NGP_F16)
    assert B >= 16384 and capi.lib.ngp_grid_backward_workspace_bytes(arr, *args) > 0, 'some level is sorted'
    assert capi.lib.ngp_grid_table_adam_prefix(arr, *args) == 0xffffffff, 'some level is not'
    # and it is the 4096-entry level alone that is sorted: the workspace is that of the one-level table
    small = np.array([0, 4096], np.int32)
    assert capi.lib.ngp_grid_backward_workspace_bytes(arr, *args) == \
        capi.lib.ngp_grid_backward_workspace_bytes(ctypes.cast(_host(small), ctypes.c_void_p), B, case.D, C, 1, S, case.H, case.gridtype, int(case.align), capi.NGP_F16)
    sorted_runs = _check_exact(case, use_workspace=True)
    assert all(nbytes > 0 for _, nbytes in sorted_runs)
    atomic_runs = _check_exact(case, use_workspace=False)
    for (a, _), (b, _) in zip(sorted_runs, atomic_runs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# (e) ray-ordered samples off the lattice: long runs on realistic fractions, every index mode once.  Per entry e with n_e hits and
# A_e = sum|contribution| (both from the oracle), eps = 2^-24 (fp32) or 2^-11 (fp16):
#     |got_e - ref_e| <= A_e * ((D + 2) * 2^-24 + n_e * eps)
# (D + 1 fp32 roundings of w * g and one for the run sum; one rounding to the table type per add, of a partial sum that is <= A_e)
# (glc.ray_case says how the fp16 case keeps every contribution in fp16's normal range, where a rounding IS relative)
@pytest.mark.parametrize('D,C,dtype,gridtype,align,interp,log2_size', glc.RAY_CASES)
def test_ray_ordered_samples_within_the_rounding_bound(D, C, dtype, gridtype, align, interp, log2_size):
    rc = glc.ray_case(D, C, dtype, gridtype, align, interp, log2_size)
    ref, A, hits = rc['ref'], rc['A'], rc['hits']
    got, _ = _backward(rc['x'], rc['g'], rc['offs'], rc['S'], rc['H'], dtype, gridtype, align, interp)
    got = got.double().numpy()
    eps = 2.0 ** -11 if dtype == 'f16' else 2.0 ** -24
    bound = A * ((D + 2) * 2.0 ** -24 + hits[:, None] * eps)
    err = np.abs(got - ref)
    print('max err / bound: %.3g; max err %.3g; longest hit list %d' % (np.max(err[bound > 0] / bound[bound > 0]), err.max(), hits.max()))
    assert np.all(got[hits == 0] == 0), 'untouched entries stay exactly zero'
    assert np.all(err <= bound)


# (f) grad_total_variation: k_grad_tv<T, D, C> over (D, C), hash / tiled, align_corners, fp32 / fp16 (odd C: a CAS per value, even C:
# a CAS per pair).  Points at 0 and 1 in every coordinate reach `cur > 0`, `cur < resolution` and the align_corners wrap.
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('gridtype', [0, 1])
@pytest.mark.parametrize('D,C', [(2, 1), (2, 8), (3, 1), (3, 4), (4, 2), (5, 2)])
def test_grad_total_variation_over_its_space(D, C, gridtype, align, dtype):
    """fp32: the tolerance of the existing test.  fp16: per entry n_e * 2^-11 * (|g0_e| + sum|update|_e) + 2e-4 * sum|update|_e, i.e. ONE
    rounding to fp16 per add.  Both fp16 paths add in fp32 inside a 32-bit CAS and round once: one value per word with odd C, a pair with
    even C.  (The packed fp16 atomic of the backward takes an fp16 addend -- the update rounded, then the sum rounded again; a host model of
    that on these inputs left the bound on single-hit entries in 6 of the 12 even-C cases, err / bound up to 1.17, so k_grad_tv does not use it.)"""
    capi = _capi()
    rng = np.random.default_rng(1000 * D + 100 * C + 10 * gridtype + int(align))
    offs, _ = oracle.grid_offsets(input_dim=D, num_levels=3, level_dim=C, per_level_scale=2, base_resolution=4, log2_hashmap_size=9,
                                  align_corners=align)
    S, H, L, B, weight = 1.0, 4, 3, 2048, 1e-2
    emb = rng.uniform(-1, 1, (int(offs[-1]), C)).astype(np.float32)
    g0 = rng.normal(size=emb.shape).astype(np.float32) * 1e-3
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[0], x[1] = 0.0, 1.0
    for d in range(D):
        x[2 + 2 * d, d], x[3 + 2 * d, d] = 0.0, 1.0
    x[20] = np.nextafter(np.float32(1.0), np.float32(2.0))
    x[21, 0] = -1e-7
    if dtype == 'f16':     # the kernel reads positions, table and gradient in the table type
        emb, g0, x = oracle.round_fp16(emb), oracle.round_fp16(g0), oracle.round_fp16(x)
    xt = torch.from_numpy(x).cuda().to(TORCH[dtype])
    et = torch.from_numpy(emb).cuda().to(TORCH[dtype])
    gt = torch.from_numpy(g0).cuda().to(TORCH[dtype])
    ot = torch.from_numpy(offs).cuda()
    capi.check(capi.lib.ngp_grad_total_variation(xt.data_ptr(), et.data_ptr(), gt.data_ptr(), ot.data_ptr(), weight, B, D, C, L, S, H, gridtype,
                                                 int(align), _code(dtype), capi.stream()))
    torch.cuda.synchronize()
    got = gt.cpu().double().numpy()
    ref = oracle.grid_grad_tv(x, emb, g0, offs, weight, S, H, gridtype=gridtype, align_corners=align)
    assert np.abs(ref - g0).max() > 1e-4, 'the update is not vacuous'
    if dtype == 'f32':
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-6)   # the tolerance of test_gpu_grid.py::test_grad_total_variation
        return
    # fp16: one rounding to fp16 per add, of a partial sum that is <= |g0_e| + sum|update|_e, plus 2e-4 relative on the updates (fp32
    # arithmetic and rsqrt: the figure of the fp32 case).  sum|update|_e: the oracle on one sample at a time; n_e: hits of the cell index.
    U = np.zeros_like(ref)
    zero = np.zeros_like(g0)
    for b in range(B):
        U += np.abs(oracle.grid_grad_tv(x[b:b + 1], emb, zero, offs, weight, S, H, gridtype=gridtype, align_corners=align))
    idx = oracle.grid_corner_indices(x, offs, S, H, gridtype, align)[:, :, 0]
    hits = np.zeros(int(offs[-1]), np.int64)
    for l in range(L):
        row = idx[l][idx[l] != 0xFFFFFFFF].astype(np.int64)
        hits[offs[l]:offs[l + 1]] = np.bincount(row, minlength=int(offs[l + 1] - offs[l]))
    assert np.all(U[hits == 0] == 0) and np.all(U >= np.abs(ref - g0) * (1 - 1e-12))
    bound = hits[:, None] * 2.0 ** -11 * (np.abs(g0) + U) + 2e-4 * U
    err = np.abs(got - ref)
    print('max err / bound: %.3g; max err %.3g; most hits %d' % (np.max(err[bound > 0] / bound[bound > 0]), err.max(), hits.max()))
    assert np.array_equal(got[hits == 0], g0[hits == 0].astype(np.float64)), 'untouched entries keep their value'
    assert np.all(err <= bound)
