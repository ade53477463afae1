"""GPU: the training step replayed from a native command list (csrc/cmdlist.cpp, graph.GraphedTrainStep) is the step replayed from its HIP
graph, bit for bit -- NeRFNetwork(bound=1, cuda_ray=True) on the synthetic scene with 512 rays per step (~33 k samples: the table's Adam
sweep needs >= 16 384, capacities come in quanta of 8192).  Every run is 16 eager steps (the sample estimate does not exist before the
first occupancy refresh) and 20 replayed ones, which cross the refresh at step 32 where the lookahead is suspended and resumed.  The
reference of every comparison is the same schedule with NGP_STEP_CMDLIST=0 (the graph replay), computed once per schedule."""
import pytest
import torch

import oracle
import synthetic_scene as sc

pytestmark = pytest.mark.gpu

N_RAYS = 512
N_STEPS = 36
KW = dict(staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
STANDING_SCALE = 128.0   # every step of these schedules stands (the default 2^16 would overflow and skip a few first steps)
SKIPPED_STEP = 22
# the main chain of the lookahead step with the table's Adam in the grid backward, as the kernel timeline shows it
# (grid forward, network forward, composite + loss + backward, colour backward, sigma backward, record sort, slice accumulate with the
# table's Adam and the carried reductions, the closing Adam / commit launch)
CHAIN = ('k_grid_forward_fast', 'k_network_forward', 'k_composite_train_loss_bwd', 'k_ffmlp_backward_paired', 'k_ffmlp_backward_paired',
         'k_grid_backward_bin', 'k_grid_backward_accumulate', 'k_adam_small_commit')

_SHARED = {}


def _scene(dev):
    if 'scene' not in _SHARED:
        occ = torch.from_numpy(sc.occupancy_density()).to(dev)
        bits = torch.from_numpy(oracle.packbits(sc.occupancy_density(), 10.0)).to(dev)
        batches = []
        for i in range(N_STEPS + 1):
            o, d, gt = sc.training_batch(N_RAYS, seed=1300 + i)
            batches.append((torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)))
        bad = batches[SKIPPED_STEP][2].clone()
        bad[:, 1] = float('inf')   # (every ray: a ray that meets no sample hands its error to nobody)
        _SHARED['scene'] = (occ, bits, batches, bad)
    return _SHARED['scene']


def _make_ngp(dev):
    import raymarching
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    model.train()
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.iter_density = 16
    opt = NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    opt.scalars[0] = STANDING_SCALE
    return model, opt


def _run(monkeypatch, schedule, lookahead=True, lists=True, march_at=None, keep=False, perturb=False):
    """one training run; schedule: 'plain', 'skip' (one batch whose target holds an inf) or 'ladder' (the sample estimate moves to another
    captured capacity and back).  -> (what must be equal as bits, the stepper's own figures[, the stepper])"""
    from graph import GraphedTrainStep
    dev = torch.device('cuda')
    occ, bits, batches, bad = _scene(dev)
    monkeypatch.setenv('NGP_STEP_CMDLIST', '1' if lists else '0')
    if march_at is None:
        monkeypatch.delenv('NGP_STEP_MARCH_AT', raising=False)
    else:
        monkeypatch.setenv('NGP_STEP_MARCH_AT', march_at)

    def keep_scene(m):
        m.density_grid.copy_(occ)
        m.density_bitfield.copy_(bits)

    model, opt = _make_ngp(dev)
    st = GraphedTrainStep(model, opt, None, N_RAYS, dict(KW, perturb=perturb), after_update=keep_scene, direct=True, lookahead=lookahead, fused_table_adam=True,
                          capacity_ladder=(1.5, 2.0) if schedule == 'ladder' else ())
    losses = []
    for i in range(N_STEPS):
        o, d, t = batches[i]
        if schedule == 'skip' and i == SKIPPED_STEP:
            t = bad
        if schedule == 'ladder':
            if i == 18:
                st.precapture()
            if i in (20, 27):          # the estimate nearly doubles, later comes back: past the hysteresis of the captured buffer both ways
                model.mean_count = int(model.mean_count * (1.9 if i == 20 else 1 / 1.9))
        nxt = batches[i + 1]
        if schedule == 'skip' and i + 1 == SKIPPED_STEP:
            nxt = (nxt[0], nxt[1], bad)
        losses.append(st.step(o, d, t, **(dict(next_rays=nxt) if lookahead else {})).detach().clone().view(1))
    assert st.capture_error is None and st.n_captures >= 1 and st.used_direct and st.table_fused
    torch.cuda.synchronize()              # (the last step's lookahead writes the ring on the side stream)
    ring = model.step_counter.clone()
    scalars_raw = opt.scalars.clone()     # (before sync_params: the parity word as the steps left it)
    st.sync_params()
    emb, ws, wc = model.encoder.embeddings, model.sigma_net.weights, model.color_net.weights
    state = dict(losses=torch.cat(losses), ring=ring, emb=emb, emb_m=opt.state[emb]['exp_avg'], emb_v=opt.state[emb]['exp_avg_sq'],
                 emb16=emb._ngp_fp16, sigma=ws, sigma_m=opt.state[ws]['exp_avg'], sigma_v=opt.state[ws]['exp_avg_sq'], color=wc,
                 color_m=opt.state[wc]['exp_avg'], color_v=opt.state[wc]['exp_avg_sq'],
                 scalars=scalars_raw[[0, 1, 3, 5]])   # scale, growth tracker, step count, parity
    state = {k: v.detach().clone() for k, v in state.items()}
    figures = dict(list_replays=st.n_list_replays, la_hits=st.la_hits, switches=st.n_switches, captured=sorted(st._captured),
                   lists_per_capacity={c: snap.get('lists') for c, snap in st._captured.items()})
    if keep:
        return state, figures, st
    st.close()
    return state, figures


def _reference(monkeypatch, schedule, lookahead=True, perturb=False):
    key = (schedule, lookahead, perturb)
    if key not in _SHARED:
        state, figures = _run(monkeypatch, schedule, lookahead, lists=False, perturb=perturb)
        assert figures['list_replays'] == 0 and all(v is None for v in figures['lists_per_capacity'].values())
        _SHARED[key] = state
    return _SHARED[key]


def _assert_same_bits(got, want):
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        view = {4: torch.int32, 2: torch.int16}[a.element_size()]
        assert torch.equal(a.view(view), b.view(view)), f'{k} differs from the graph replay'


# without the lookahead the march is part of the chain: the marcher draws its start offsets itself (perturb=True, seeded by the step count)
@pytest.mark.parametrize('lookahead,perturb', [(True, False), (True, True), (False, True)])
def test_list_replay_is_the_graph_replay_bit_for_bit(monkeypatch, lookahead, perturb):
    want = _reference(monkeypatch, 'plain', lookahead, perturb)
    got, figures = _run(monkeypatch, 'plain', lookahead, perturb=perturb)
    assert figures['list_replays'] == N_STEPS - 16                    # every replayed step went through its list
    if lookahead:
        assert figures['la_hits'] >= N_STEPS - 16 - 3                 # all but the steps around the refresh were marched ahead
    assert float(want['scalars'][2]) == N_STEPS                       # (no step was skipped)
    _assert_same_bits(got, want)


def test_a_chain_with_a_torch_kernel_keeps_the_graph_replay(monkeypatch):
    """no lookahead, perturb=False: the captured march reads a torch.zeros tensor that is filled inside the capture -- not eligible"""
    got, figures = _run(monkeypatch, 'plain', lookahead=False)
    assert figures['list_replays'] == 0 and all(v is None for v in figures['lists_per_capacity'].values())
    assert float(got['scalars'][2]) == N_STEPS and bool(torch.isfinite(got['losses']).all())


def test_a_skipped_step_behaves_as_in_the_graph_form(monkeypatch):
    want = _reference(monkeypatch, 'skip')
    got, figures = _run(monkeypatch, 'skip')
    assert figures['list_replays'] == N_STEPS - 16
    plain = _reference(monkeypatch, 'plain')
    # found_inf was raised: one step less stands and the scale backed off
    assert float(want['scalars'][2]) == N_STEPS - 1 and float(want['scalars'][0]) < float(plain['scalars'][0])
    assert not bool(torch.isfinite(want['losses'][SKIPPED_STEP])) and bool(torch.isfinite(want['losses'][SKIPPED_STEP + 1:]).all())
    _assert_same_bits(got, want)                                      # the skipped step, and every good step behind it


def test_each_capacity_replays_its_own_list(monkeypatch):
    want = _reference(monkeypatch, 'ladder')
    got, figures = _run(monkeypatch, 'ladder')
    assert figures['switches'] >= 2 and len(figures['captured']) >= 3
    lists = figures['lists_per_capacity']
    assert all(v is not None and len(v) == 2 for v in lists.values())             # per capacity: one list per buffer set
    assert len({id(cl) for v in lists.values() for cl in v}) == 2 * len(lists)
    assert figures['list_replays'] == N_STEPS - 16
    _assert_same_bits(got, want)


def test_recorded_chain_and_its_lifetime(monkeypatch):
    """the list holds exactly the launches of the main chain, in order; close() destroys it ahead of the graph that owns its buffers"""
    want = _reference(monkeypatch, 'plain')
    got, figures, st = _run(monkeypatch, 'plain', keep=True)
    try:
        assert st.lists is not None and len(st.lists) == 2 and len(st.graphs) == 4
        for cl in st.lists:
            names = cl.names()
            assert len(names) == len(CHAIN), names
            for name, kernel in zip(names, CHAIN):
                assert kernel in name, (name, kernel)
        held = st.lists[0]
    finally:
        st.close()
    assert st.lists is None and held.handle is None
    with pytest.raises(RuntimeError, match='the list is NULL or was destroyed'):
        held.replay(torch.cuda.current_stream().cuda_stream)
    _assert_same_bits(got, want)


@pytest.mark.parametrize('march_at', ['net', 'composite', 'sigma', 'sort'])
def test_march_placement_is_scheduling_only(monkeypatch, march_at):
    want = _reference(monkeypatch, 'plain')
    got, figures = _run(monkeypatch, 'plain', march_at=march_at)
    assert figures['list_replays'] == N_STEPS - 16 and figures['la_hits'] >= N_STEPS - 16 - 3
    _assert_same_bits(got, want)


def test_unknown_march_placement_is_refused(monkeypatch):
    from graph import GraphedTrainStep
    monkeypatch.setenv('NGP_STEP_MARCH_AT', 'nowhere')
    model, opt = _make_ngp(torch.device('cuda'))
    with pytest.raises(ValueError, match='NGP_STEP_MARCH_AT'):
        GraphedTrainStep(model, opt, None, N_RAYS, KW, direct=True, lookahead=True)
