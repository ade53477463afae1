"""GPU: the training step whose per-sample kernels stop at the rows the march filled (fused.USE_ROW_BOUND, include/ngp_hip.h
ngp_training_row_bound) is the capacity-sized step -- the schedules of tests/test_gpu_step_cmdlist.py (512 rays, 16 eager + 20 replayed steps
across an occupancy refresh), each run once with the bound and once without it: with and without lookahead, with one skipped step (`inf`
target) and across a capacity switch.  Losses, the sample-count ring, table / moments / fp16 shadow, both MLPs with their moments, scale,
growth tracker, step count and parity must be equal BY VALUE (-0 == +0, NaNs in the same places); a difference that is only the sign of a
zero is reported with its position."""
import pytest
import torch

import test_gpu_step_cmdlist as base

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _run(monkeypatch, bound, schedule, lookahead, perturb):
    import fused
    monkeypatch.setattr(fused, 'USE_ROW_BOUND', bound)
    state, figures = base._run(monkeypatch, schedule, lookahead, perturb=perturb)
    return state, figures


def _unbounded(monkeypatch, schedule, lookahead, perturb):
    key = (schedule, lookahead, perturb)
    if key not in _REFERENCE:
        _REFERENCE[key] = _run(monkeypatch, False, schedule, lookahead, perturb)
    return _REFERENCE[key]


def _assert_same_values(got, want):
    zero_sign_only = []
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        af, bf = a.double().flatten(), b.double().flatten()
        nan_a, nan_b = torch.isnan(af), torch.isnan(bf)
        assert torch.equal(nan_a, nan_b), f'{k}: NaNs in other places than in the capacity-sized step'
        differs = (af != bf) & ~nan_a
        assert not bool(differs.any()), f'{k}: {int(differs.sum())} values differ from the capacity-sized step, first at {int(differs.nonzero()[0])}'
        signs = (torch.signbit(af) != torch.signbit(bf)) & ~nan_a
        if bool(signs.any()):
            zero_sign_only.append((k, int(signs.sum()), int(signs.nonzero()[0])))
    if zero_sign_only:
        print('equal by value; zeros of the other sign (tensor, count, first index):', zero_sign_only)


# (without the lookahead the march is part of the chain and draws its start offsets itself: perturb=True, tests/test_gpu_step_cmdlist.py)
@pytest.mark.parametrize('schedule,lookahead,perturb', [('plain', True, False), ('plain', False, True), ('skip', True, False), ('ladder', True, False)])
def test_bounded_step_is_the_capacity_sized_step(monkeypatch, schedule, lookahead, perturb):
    want, want_fig = _unbounded(monkeypatch, schedule, lookahead, perturb)
    got, got_fig = _run(monkeypatch, True, schedule, lookahead, perturb)
    # the same replays of the same lists: the bound is a kernel parameter of the chain's launches, not another chain
    assert got_fig['list_replays'] == want_fig['list_replays'] == base.N_STEPS - 16
    assert got_fig['switches'] == want_fig['switches'] and got_fig['captured'] == want_fig['captured']
    if schedule == 'skip':
        assert float(want['scalars'][2]) == base.N_STEPS - 1 and not bool(torch.isfinite(want['losses'][base.SKIPPED_STEP]))
    else:
        assert float(want['scalars'][2]) == base.N_STEPS and bool(torch.isfinite(want['losses']).all())
    if schedule == 'ladder':
        assert got_fig['switches'] >= 2
    # the last 16 steps' sample counts against the captured buffers: in some steps the bound lies below the capacity (a real bound), in
    # others the samples fill the buffer and the bound is the capacity -- printed, and the real-bound case asserted
    ring = want['ring'][:, 0]
    print('samples of the last 16 steps', ring.tolist(), 'captured capacities', want_fig['captured'])
    assert int(ring.min()) + 512 < max(want_fig['captured']), (ring.tolist(), want_fig['captured'])
    _assert_same_values(got, want)


def test_the_bounded_chain_is_the_same_launches(monkeypatch):
    """the bound adds no kernel: the recorded chain has the names and the count tests/test_gpu_step_cmdlist.py lists"""
    import fused
    monkeypatch.setattr(fused, 'USE_ROW_BOUND', True)
    _, _, st = base._run(monkeypatch, 'plain', keep=True)
    try:
        assert st.lists is not None and len(st.lists) == 2
        for cl in st.lists:
            names = cl.names()
            assert len(names) == len(base.CHAIN), names
            for name, kernel in zip(names, base.CHAIN):
                assert kernel in name, (name, kernel)
    finally:
        st.close()
