"""GPU checks of the occupancy kernels through raymarching.raymarching._backend (the binding over the C ABI of include/ngp_hip.h that the
operators themselves call: the compiled module where it is built, the ctypes one otherwise), on the tables of tests/occupancy_cases.py and
against its models (tests/test_occupancy_cases.py checks those on the CPU):

  ngp_density_grid_update (k_density_scatter, k_density_apply_mean, k_packbits)  against density_update_model
  ngp_packbits / ngp_packbits_ex / ngp_packbits_f64                              against packbits_model
  ngp_coarse_occupancy                                                           against coarse_model
  ngp_cull_rays                                                                  against cull_model (oracle.cull_rays), ray for ray

Every comparison is exact -- grids bit for bit, bitfields, coarse grids and verdicts byte for byte -- with one exception, the mean of a
grid whose double sum is not exact in every order (see _check_mean).  No network is built anywhere."""
import numpy as np
import pytest
import torch

import oracle
import occupancy_cases as O

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 0xA5


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rb():
    from raymarching.raymarching import _backend as rb
    return rb


def _i32(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------
# ngp_density_grid_update
# ------------------------------------------------------------------------------------------------
class _State:
    """the buffers of one occupancy grid as the renderer keeps them: scratch at -1, the workspace zeroed ONCE.  scratch has OOB spare floats
    behind the n_cells the kernel is told about, holding a sentinel: a scatter without its index guard changes them (a failed assertion)
    and writes nothing outside the allocation."""

    def __init__(self, grid0):
        rb = _rb()
        self.n_cells = len(grid0)
        self.grid = cu(grid0)
        self.scratch = torch.full((self.n_cells + O.OOB,), -1.0, dtype=torch.float32, device='cuda')
        self.scratch[self.n_cells:] = O.SENTINEL
        self.mean = torch.full((4,), O.SENTINEL, dtype=torch.float32, device='cuda')
        self.bitfield = torch.full((self.n_cells // 8 + 16,), GUARD, dtype=torch.uint8, device='cuda')
        self.workspace = torch.zeros(rb.density_grid_update_workspace_bytes(self.n_cells), dtype=torch.uint8, device='cuda')

    def update(self, sigmas, cells, scale, decay, thresh):
        """-> grid, mean, bitfield after the call (numpy), having checked everything around them"""
        s, c = cu(sigmas), cu(cells)
        _rb().density_grid_update(s, c, len(cells), scale, decay, self.grid, self.n_cells, self.scratch, thresh, self.mean, self.bitfield,
                                  self.workspace)
        torch.cuda.synchronize()
        scratch = self.scratch.cpu().numpy()
        assert np.array_equal(_i32(scratch[:self.n_cells]), _i32(np.full(self.n_cells, -1.0, F32))), 'scratch is -1.0 everywhere after the call'
        assert (scratch[self.n_cells:] == O.SENTINEL).all(), 'an index >= n_cells was written'
        mean = self.mean.cpu().numpy()
        assert (mean[1:] == O.SENTINEL).all()
        bitfield = self.bitfield.cpu().numpy()
        assert (bitfield[self.n_cells // 8:] == GUARD).all()
        return self.grid.cpu().numpy(), mean[0], bitfield[:self.n_cells // 8]


def _check_grid(got, before, ref, what):
    """the grid lies within the admissible sets: bit-equal to the model wherever a cell was sampled at most once (untouched cells and
    cells < 0 keep their bits: the model leaves them alone), one of the cell's admissible values where it was sampled several times"""
    several = np.array(sorted(ref['admissible']), np.int64)
    once = np.ones(len(got), bool)
    once[several] = False
    assert np.array_equal(_i32(got)[once], _i32(ref['grid'])[once]), (what, np.nonzero(_i32(got) != _i32(ref['grid']))[0][:8])
    for cell in several:
        assert int(_i32(got[cell:cell + 1])[0]) in ref['admissible'][int(cell)], (what, int(cell), got[cell])
    sampled = np.zeros(len(got), bool)
    sampled[ref['sampled']] = True
    assert np.array_equal(_i32(got)[~sampled], _i32(before)[~sampled]), (what, 'an untouched cell changed')
    assert np.array_equal(_i32(got)[before < 0], _i32(before)[before < 0]), (what, 'a cell < 0 changed')


def _check_mean(mean, grid, exact, what):
    """the kernel's mean against float32(exact sum of max(g, 0) / n_cells) of ITS OWN grid (which of several samples won is its choice).
    `exact` (the dyadic tables: every partial sum is a multiple of 2^-13 below 2^41, exact in a double in any order): bit for bit.
    Otherwise at most 1 fp32 ulp apart: the kernel adds n_cells non-negative doubles, each addition off by at most 2^-53 relative, so its
    quotient is within (n_cells + 1) 2^-53 <= 2.4e-10 of the exact mean; the model's (the correctly rounded sum, divided) within 2.3e-16.
    Both are rounded to fp32 once more.  Two doubles 2.4e-10 apart -- 1/250 of an fp32 half-ulp -- round to the same float or, when a
    rounding boundary lies between them, to two neighbouring ones: never further apart."""
    want = O.mean_of(grid)
    print(f'{what}: mean {float(mean)!r}, exact {float(want)!r}')
    if exact or not np.isfinite(want):
        assert _i32(mean) == _i32(want), (what, float(mean), float(want))
    else:
        assert mean >= 0 and O.ulps_apart(mean, want) <= 1, (what, float(mean), float(want))


@pytest.mark.parametrize('kind', O.UPDATE_KINDS)
@pytest.mark.parametrize('n_cells', O.UPDATE_CELLS)
def test_density_grid_update_equals_the_model_call_after_call(kind, n_cells):
    """the four consecutive calls of the table on ONE state (every cell once + specials + out-of-range indices; duplicate groups; n = 0; a few
    cells, one of them +inf): each call's grid, scratch, mean and bitfield.  The workspace is zeroed once, before the first call: a ticket
    that is not handed back, or a partial left over from another call, shows in the next call's mean."""
    t = O.update_table(kind, n_cells)
    st = _State(t['grid0'])
    before = t['grid0']
    for i, (sigmas, cells) in enumerate(t['calls']):
        what = f'{kind} {n_cells} call {i}'
        ref = O.density_update_model(before, True, sigmas, cells, t['scale'], t['decay'], t['thresh'])
        grid, mean, bitfield = st.update(sigmas, cells, t['scale'], t['decay'], t['thresh'])
        _check_grid(grid, before, ref, what)
        _check_mean(mean, grid, kind == 'dyadic', what)
        used = min(F32(t['thresh']), mean)
        if kind != 'dyadic':    # the table's promise, on the grid as it came out: a mean 1 ulp off packs the same bits
            assert O.cells_near(grid, min(F32(t['thresh']), O.mean_of(grid))) == 0
        assert np.array_equal(bitfield, oracle.packbits(grid, float(used))), what
        assert np.array_equal(bitfield, O.packbits_model(grid, t['thresh'], float(O.mean_of(grid)))), what
        before = grid           # the next call starts from what the kernel left (its choice among duplicates included)
    # the cap of ngp_packbits_ex may be the mean of this very state
    out = torch.full((n_cells // 8 + 16,), GUARD, dtype=torch.uint8, device='cuda')
    _rb().packbits_capped(st.grid, n_cells // 8, t['thresh'], st.mean, out)
    torch.cuda.synchronize()
    assert torch.equal(out, st.bitfield)


@pytest.mark.parametrize('n_cells', (8, O.BLOCK + 8, 257 * O.BLOCK + 8))
def test_density_grid_update_repeats_its_mean_bit_for_bit(n_cells):
    """two states with equal inputs: the same grid and the same mean bits (a fixed summation order), on the table whose sum is NOT exact"""
    t = O.update_table('generic', n_cells)
    sigmas, cells = t['calls'][0]
    runs = []
    for _ in range(2):
        st = _State(t['grid0'])
        for _ in range(2):      # (the second call works on what the first one left, ticket and partials included)
            grid, mean, bitfield = st.update(sigmas, cells, t['scale'], t['decay'], t['thresh'])
        runs.append((grid, mean, bitfield))
    assert np.array_equal(_i32(runs[0][0]), _i32(runs[1][0])) and _i32(runs[0][1]) == _i32(runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


# ------------------------------------------------------------------------------------------------
# packbits
# ------------------------------------------------------------------------------------------------
def test_packbits_on_the_threshold_cases():
    rb = _rb()
    for case in O.packbits_cases():
        N = len(case['grid']) // 8
        want = O.packbits_model(case['grid'], case['thresh'], case['cap'])
        grid = cu(case['grid'])
        out = torch.full((N + 16,), GUARD, dtype=torch.uint8, device='cuda')
        if case['cap'] is None:     # ngp_packbits: ngp_packbits_ex without a cap
            rb.packbits(grid, N, case['thresh'], out)
        else:
            rb.packbits_capped(grid, N, case['thresh'], cu(np.array([case['cap'], 1e30], F32)), out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:N], want) and (got[N:] == GUARD).all(), case['name']


def test_packbits_f64_compares_in_double():
    grid, thresh = O.packbits_f64_case()
    N = len(grid) // 8
    out = torch.full((N + 16,), GUARD, dtype=torch.uint8, device='cuda')
    _rb().packbits(cu(grid), N, thresh, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:N], O.packbits_model(grid, thresh)) and (got[N:] == GUARD).all()
    assert not np.array_equal(got[:N], O.packbits_model(grid.astype(F32), thresh))


# ------------------------------------------------------------------------------------------------
# coarse occupancy
# ------------------------------------------------------------------------------------------------
def _coarse(bits, C, H, extra=64):
    """-> the kernel's coarse grid (device tensor of exactly C (H/4)^3 bytes), having checked that the bytes behind it are untouched"""
    n = C * (H // 4) ** 3
    buf = torch.full((n + extra,), GUARD, dtype=torch.uint8, device='cuda')
    _rb().coarse_occupancy(cu(bits), C, H, buf)
    torch.cuda.synchronize()
    assert (buf[n:] == GUARD).all()
    return buf[:n].clone()


@pytest.mark.parametrize('H,C', O.COARSE_GRIDS)
def test_coarse_occupancy_equals_the_model(H, C):
    import _ngp_capi as capi
    assert int(capi.lib.ngp_coarse_occupancy_bytes(C, H)) == C * (H // 4) ** 3
    for fill in O.COARSE_FILLS:
        bits = O.coarse_fill(fill, C, H)
        got = _coarse(bits, C, H).cpu().numpy()
        want = O.coarse_model(bits, C, H)
        assert np.array_equal(got, want), (fill, np.nonzero(got != want)[0][:8])


# ------------------------------------------------------------------------------------------------
# cull
# ------------------------------------------------------------------------------------------------
def _cull(o, d, nears, fars, bound, C, H, coarse, N=None, tail=40):
    """-> flags [N] of the first N rays, having checked that the `tail` entries behind them keep their sentinel"""
    N = len(nears) if N is None else N
    flags = torch.full((N + tail,), 7, dtype=torch.int32, device='cuda')
    _rb().cull_rays(cu(o), cu(d), cu(nears), cu(fars), N, bound, C, H, coarse, flags)
    torch.cuda.synchronize()
    flags = flags.cpu().numpy()
    assert (flags[N:] == 7).all(), 'rays_alive[N:] was written'
    return flags[:N]


def test_cull_gives_the_named_rays_their_stated_verdict():
    bound, C, H = O.NAMED_GRID
    for fill in ('empty', 'full'):
        names, o, d, nears, fars, kept = O.named_rays(fill)
        flags = _cull(o, d, nears, fars, bound, C, H, _coarse(O.coarse_fill(fill, C, H), C, H))
        for i, name in enumerate(names):
            assert flags[i] == (i if kept[i] else -1), (name, flags[i])


@pytest.mark.parametrize('bound,C,H', O.CULL_CONFIGS)
def test_cull_verdicts_equal_the_model_for_every_ray(bound, C, H):
    """ngp_cull_rays on the kernel's own coarse grid against the fp32 model on the model's: the same verdict for every one of the 20 000
    rays and of the prefixes of 1, 255, 256 and 257 -- no tolerance, no ray left out: both sides perform the same correctly rounded fp32
    operations.  Kept rays carry their own index."""
    t = O.cull_table(bound, C, H)
    coarse = _coarse(t['bits'], C, H)
    assert np.array_equal(coarse.cpu().numpy(), t['coarse'])
    want = O.cull_model(t['o'], t['d'], t['nears'], t['fars'], bound, C, H, t['coarse'])
    for N in O.CULL_SIZES + (O.CULL_N,):
        got = _cull(t['o'], t['d'], t['nears'], t['fars'], bound, C, H, coarse, N=N)
        differ = np.nonzero(got != want[:N])[0]
        assert len(differ) == 0, (N, len(differ), differ[:8], got[differ[:8]], want[differ[:8]])
        kept = got >= 0
        assert np.array_equal(got[kept], np.arange(N, dtype=np.int32)[kept]) and (got[~kept] == -1).all()


@pytest.mark.parametrize('bound,C,H', [c for c in O.CULL_CONFIGS if c[2] in (16, 32)])
def test_no_culled_ray_emits_a_sample_from_the_marcher(bound, C, H):
    """the direct cross-check: what ngp_cull_rays drops, the GPU marcher (n_step = 1, every ray alive, t from near) emits nothing for"""
    import raymarching as rm
    t = O.cull_table(bound, C, H)
    N = O.CULL_N
    culled = _cull(t['o'], t['d'], t['nears'], t['fars'], bound, C, H, _coarse(t['bits'], C, H)) < 0
    to, td, tn, tf, tb = cu(t['o']), cu(t['d']), cu(t['nears']), cu(t['fars']), cu(t['bits'])
    alive = torch.arange(N, dtype=torch.int32, device='cuda')
    for dt_gamma in O.DT_GAMMAS:
        x, dd, de = rm.march_rays(N, 1, alive, tn.clone(), to, td, bound, tb, C, H, tn, tf, 128, False, dt_gamma, 1024)
        emits = (de[:N, 0] > 0).cpu().numpy()
        assert emits.sum() > 0 and culled.sum() > 0
        assert not (culled & emits).any(), (dt_gamma, int((culled & emits).sum()))
