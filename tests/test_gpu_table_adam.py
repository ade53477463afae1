"""GPU: the hash table's Adam sweep INSIDE the grid backward's slice accumulate (round 6; include/ngp_hip.h ngp_table_adam_t,
optim.NGPAdam.enable_table_fusion, graph.GraphedTrainStep(fused_table_adam=True)).

The reference's step is torch.optim.Adam behind GradScaler.step (nerf/utils.py:751-753): a non-finite gradient ANYWHERE skips the whole
step.  The fused form updates speculatively into a second buffer set and flips a device-side parity word only when the step stands, so it
must be the SAME training as the separate sweep (k_adam over the stored fp16 gradient), bit for bit -- parameters, moments, fp16 shadows,
loss scale, step count -- including skipped steps, and the torch Parameter must be current again after materialize().

The second half of the module looks at the table from OUTSIDE the captured graphs (checkpoints, state_dict, sync_params, the EMA, an inference
frame, the drop-in encoder; an unfused step, a checkpoint load, EMA weights written for an evaluation) after odd and even numbers of replayed
steps that stand: a replay flips the parity word on the device and Python, which ran at capture time only, has to be told
(optim.replayed_fused_table_step).  The reference of every comparison is the same training with the separate sweep, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import synthetic_scene as sc

pytestmark = pytest.mark.gpu


def _table_setup(dev, seed):
    from gridencoder import GridEncoder
    from optim import NGPAdam
    torch.manual_seed(seed)
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048).to(dev)
    with torch.no_grad():
        enc.embeddings.uniform_(-0.5, 0.5)
    small = torch.nn.Parameter(torch.randn(7168, device=dev) * 0.1)
    opt = NGPAdam([{'params': [enc.embeddings], 'lr': 1e-2}, {'params': [small], 'lr': 3e-3}], betas=(0.9, 0.99), eps=1e-15, init_scale=128.0,
                  growth_interval=2)
    return enc, small, opt


def _backward(enc, g_enc, x, opt, fused_adam):
    import _ngp_capi as capi
    import fused
    M = x.shape[0]
    S = float(np.log2(enc.per_level_scale))
    assert capi.host_offsets(enc.offsets) is not None
    emb = enc.embeddings
    fused._grid_backward(g_enc, x, enc.offsets, emb._ngp_grad16, M, 16, S, 16, enc.gridtype_id, 0, enc.interp_id, 0.0, capi.stream(),
                         found_inf=opt.scalars[2:3], slabs=None, overwrite=True, table_adam=opt.table_adam() if fused_adam else None)
    emb._ngp_deposit_overwritten = True
    if fused_adam:   # (what the fused iteration announces to the optimizer's closing launch: the dense-level prefix is its part)
        arr = capi.host_offsets(enc.offsets)
        prefix = int(capi.lib.ngp_grid_table_adam_prefix(ctypes.cast(arr, ctypes.c_void_p), M, 3, 2, 16, S, 16, enc.gridtype_id, 0, capi.NGP_F16))
        assert 0 < prefix < 0xffffffff and prefix == int(enc.offsets[5])     # levels 0-4 of the lego table are dense
        from optim import announce_overwrite
        announce_overwrite(emb, table_adam_prefix=prefix)


def test_fused_flush_is_the_separate_adam_sweep_bit_for_bit():
    dev = torch.device('cuda')
    M = 32768
    enc_a, small_a, opt_a = _table_setup(dev, 0)
    enc_b, small_b, opt_b = _table_setup(dev, 0)
    assert torch.equal(enc_a.embeddings, enc_b.embeddings)
    opt_b.enable_table_fusion(enc_b.embeddings)
    alt = opt_b._table_alt
    gen = torch.Generator(device='cuda').manual_seed(5)
    parities, skipped = [], 0
    for it in range(7):
        x = torch.rand(M, 3, device=dev, generator=gen)
        x[: M // 2] = x[: M // 2] * 0.2 + 0.4        # half of the points clustered: long same-entry runs on the coarse levels
        g_enc = (torch.randn(16, M, 2, device=dev, generator=gen) * 0.05).half()
        if it == 1:
            g_enc = (g_enc.float() * 200).half()      # contributions of ~10: slice sums beyond 128 take the other scaling of the fixed-point addend
        if it == 3:
            g_enc[7, 123, 1] = float('inf')           # a non-finite table gradient: the step is skipped as a whole
        if it == 5:
            g_enc[2].fill_(6000.0)                    # finite contributions whose SUM leaves the fp16 range on a coarse level
        gs = (torch.randn(7168, device=dev, generator=gen) * 0.01).half()
        before_b = [t.clone() for t in (enc_b.embeddings.data, opt_b.state[enc_b.embeddings]['exp_avg'], alt['p'], alt['m'])]
        parity0 = float(opt_b.scalars[5])
        for enc, small, opt, fused_adam in ((enc_a, small_a, opt_a, False), (enc_b, small_b, opt_b, True)):
            small._ngp_grad16.copy_(gs)
            _backward(enc, g_enc, x, opt, fused_adam)
            opt.step(gradients_checked=True)
        torch.cuda.synchronize()
        assert torch.equal(opt_a.scalars[:5], opt_b.scalars[:5]), (it, opt_a.scalars, opt_b.scalars)
        parity = float(opt_b.scalars[5])
        parities.append(parity)
        step_skipped = it in (3, 5)
        if step_skipped:
            skipped += 1
            assert parity == parity0                                   # a skipped step does not flip ...
            cur = (enc_b.embeddings.data, opt_b.state[enc_b.embeddings]['exp_avg']) if parity == 0 else (alt['p'], alt['m'])
            ref = (before_b[0], before_b[1]) if parity == 0 else (before_b[2], before_b[3])
            assert torch.equal(cur[0], ref[0]) and torch.equal(cur[1], ref[1])   # ... and never wrote the current set
        else:
            assert parity == 1.0 - parity0
        # the current buffer set of the fused optimizer == the separately swept one, bit for bit
        st_a, st_b = opt_a.state[enc_a.embeddings], opt_b.state[enc_b.embeddings]
        cur_b = (enc_b.embeddings.data, st_b['exp_avg'], st_b['exp_avg_sq'], st_b['fp16']) if parity == 0 else (alt['p'], alt['m'], alt['v'], alt['p16'])
        for name, ta, tb in zip(('p', 'm', 'v', 'p16'), (enc_a.embeddings.data, st_a['exp_avg'], st_a['exp_avg_sq'], st_a['fp16']), cur_b):
            assert torch.equal(ta, tb), (it, name, float((ta.float() - tb.float()).abs().max()))
        assert torch.equal(small_a.data, small_b.data) and torch.equal(small_a._ngp_fp16, small_b._ngp_fp16)
        assert torch.equal(opt_a.state[small_a]['exp_avg_sq'], opt_b.state[small_b]['exp_avg_sq'])
    assert skipped == 2 and 1.0 in parities and 0.0 in parities[1:]
    assert float(opt_a.scalars[3]) == 5.0
    # materialize: the torch Parameter and the optimizer's state are the current set again, parity 0 (step once more when A happens to be
    # current, so that the copying branch is the one exercised)
    if float(opt_b.scalars[5]) == 0.0:
        x = torch.rand(M, 3, device=dev, generator=gen)
        g_enc = (torch.randn(16, M, 2, device=dev, generator=gen) * 0.05).half()
        for enc, small, opt, fused_adam in ((enc_a, small_a, opt_a, False), (enc_b, small_b, opt_b, True)):
            small._ngp_grad16.zero_()
            _backward(enc, g_enc, x, opt, fused_adam)
            opt.step(gradients_checked=True)
    assert float(opt_b.scalars[5]) == 1.0
    assert not torch.equal(enc_a.embeddings.data, enc_b.embeddings.data)     # the Parameter is the STALE set here ...
    opt_b.materialize()
    assert float(opt_b.scalars[5]) == 0.0                                    # ... and the current one after materialize()
    st_a, st_b = opt_a.state[enc_a.embeddings], opt_b.state[enc_b.embeddings]
    assert torch.equal(enc_a.embeddings.data, enc_b.embeddings.data) and torch.equal(st_a['exp_avg'], st_b['exp_avg'])
    assert torch.equal(st_a['exp_avg_sq'], st_b['exp_avg_sq']) and torch.equal(st_a['fp16'], st_b['fp16'])
    # an UNFUSED step after fused ones keeps the two optimizers identical
    for enc, small, opt in ((enc_a, small_a, opt_a), (enc_b, small_b, opt_b)):
        enc.embeddings._ngp_grad16.fill_(0.25)
        enc.embeddings._ngp_grad16_stale = False
        enc.embeddings._ngp_deposit_overwritten = False
        small._ngp_grad16.fill_(0.5)
        opt.step()
    assert torch.equal(enc_a.embeddings.data, enc_b.embeddings.data) and torch.equal(small_a.data, small_b.data)


def test_forward_selects_the_current_copy_on_the_device():
    """ngp_grid_encode_forward_sel: the kernel reads the parity word itself"""
    import _ngp_capi as capi
    import fused
    dev = torch.device('cuda')
    enc, small, opt = _table_setup(dev, 1)
    emb = enc.embeddings
    opt.enable_table_fusion(emb)
    alt16 = opt._table_alt['p16']
    alt16.copy_((torch.randn_like(emb) * 0.3).half())
    x = torch.rand(5000, 3, device=dev) * 2 - 1
    S = float(np.log2(enc.per_level_scale))

    def run():
        out = torch.empty(16, 5000, 2, device=dev, dtype=torch.half)
        fused._grid_forward(x, emb._ngp_fp16, enc.offsets, out, 5000, 16, S, 16, enc.gridtype_id, 0, enc.interp_id, 1.0, None, capi.stream())
        return out

    def plain(table):
        out = torch.empty(16, 5000, 2, device=dev, dtype=torch.half)
        capi.check(capi.lib.ngp_grid_encode_forward_sched(x.data_ptr(), table.data_ptr(), enc.offsets.data_ptr(), out.data_ptr(), 5000, 3, 2, 16, S, 16,
                                                          None, enc.gridtype_id, 0, enc.interp_id, capi.NGP_F16, 1.0, None, capi.stream()))
        return out
    a = run()
    assert torch.equal(a, plain(emb._ngp_fp16))
    opt.scalars[5] = 1.0
    b = run()
    assert torch.equal(b, plain(alt16)) and not torch.equal(a, b)
    # the selection is made at replay time: one captured launch follows the word
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        c = run()
    for parity, table in ((0.0, emb._ngp_fp16), (1.0, alt16), (0.0, emb._ngp_fp16)):
        opt.scalars[5] = parity
        g.replay()
        assert torch.equal(c, plain(table))


def test_table_adam_is_refused_where_not_every_entry_comes_from_a_flush():
    dev = torch.device('cuda')
    enc, small, opt = _table_setup(dev, 2)
    opt.enable_table_fusion(enc.embeddings)
    M = 4096   # below the record-sort threshold: the atomic path cannot carry the sweep
    x = torch.rand(M, 3, device=dev)
    g_enc = torch.zeros(16, M, 2, device=dev, dtype=torch.half)
    before = enc.embeddings.detach().clone()
    with pytest.raises(RuntimeError, match='table_adam'):
        _backward(enc, g_enc, x, opt, True)
    torch.cuda.synchronize()
    assert torch.equal(before, enc.embeddings.detach()) and float(opt.scalars[5]) == 0.0


def _make_ngp(dev, encoder=None):
    """encoder: keyword arguments of another hash grid than the flagship one (16 levels x 2 features are what the fused iteration serves)"""
    import raymarching
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10)
    if encoder is not None:
        from gridencoder import GridEncoder
        model.encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, **encoder)
    model = model.to(dev)
    model.train()
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.iter_density = 16
    opt = NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    return model, opt


@pytest.mark.parametrize('lookahead', [True, False])
def test_graphed_training_with_fused_table_adam_is_the_same_training(lookahead, tmp_path):
    """40 steps (eager first steps, captured steps, occupancy refreshes through the double-buffered table, skipped steps from an absurd
    loss scale): bit-identical parameters, moments, losses, loss scale and step count with and without the fusion; then a checkpoint, a
    drop-in iteration and an inference frame read the table through the torch Parameter."""
    import checkpoint
    from graph import GraphedTrainStep
    dev = torch.device('cuda')
    occ = torch.from_numpy(sc.occupancy_density()).to(dev)
    bits = torch.from_numpy(oracle.packbits(sc.occupancy_density(), 10.0)).to(dev)
    n_rays = 1024
    kw = dict(staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    batches = []
    for i in range(42):
        o, d, gt = sc.training_batch(n_rays, seed=300 + i)
        batches.append((torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)))

    def keep(m):
        m.density_bitfield.copy_(bits)   # (the density grid itself follows the network: the refresh reads the table through the selection)
        m.density_grid.copy_(occ)

    runs = {}
    for fuse in (True, False):
        model, opt = _make_ngp(dev)
        opt.scalars[0] = 2.0 ** 24      # the first captured steps overflow and are skipped, alike in both modes
        st = GraphedTrainStep(model, opt, None, n_rays, kw, after_update=keep, direct=True, lookahead=lookahead, fused_table_adam=fuse)
        losses, means = [], []
        for i in range(40):
            nxt = dict(next_rays=batches[i + 1]) if lookahead else {}
            losses.append(float(st.step(*batches[i], **nxt)))
            means.append(float(model.mean_density))
        assert st.capture_error is None and st.n_captures >= 1 and st.used_direct
        assert st.table_fused == fuse
        if fuse:
            assert opt.fused_table is model.encoder.embeddings
        emb = model.encoder.embeddings
        # the Trainer's parameter EMA (torch_ema surface) reads and writes the torch Parameters: it has to see / leave the CURRENT table
        from optim import NGPEma
        ema = NGPEma([p for p in model.parameters() if p.requires_grad], 0.95, optimizer=opt)   # (reads the parameters: materializes)
        ema.update()
        ema.store()
        ema.copy_to()
        ema.restore()
        ema_sum = [float(t.double().sum()) for t in ema.shadow_params]
        state = checkpoint.save_checkpoint(str(tmp_path / f'ck_{fuse}.pth'), model, optimizer=opt, full=True)   # materializes
        assert float(opt.scalars[5]) == 0.0
        assert torch.equal(emb._ngp_fp16, emb.detach().half())
        sd = opt.state_dict()
        # one more iteration through the DROP-IN path and an unfused optimizer step
        with torch.autocast('cuda', dtype=torch.float16):
            out = model.render(batches[40][0], batches[40][1], **kw)
            loss = ((out['image'] - batches[40][2]) ** 2).mean()
        opt.scale(loss).backward()
        opt.step()
        # ... and graph steps again (the captured graphs pick the parity up where it is)
        for i in (40, 41):
            nxt = dict(next_rays=batches[(i + 1) % 42]) if lookahead else {}
            losses.append(float(st.step(*batches[i], **nxt)))
        st.sync_params()
        model.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
            frame = model.render(batches[0][0], batches[0][1], staged=False, bg_color=1, perturb=False, max_steps=1024)['image'].clone()
        params = [p.detach().clone() for p in (emb, model.sigma_net.weights, model.color_net.weights)]
        runs[fuse] = (losses, params, float(opt.scalars[0]), float(opt.scalars[3]), state['model']['encoder.embeddings'].clone(),
                      [m.clone() for m in sd['exp_avg']], means, frame, ema_sum)
        st.close()
    a, b = runs[True], runs[False]
    assert a[2] == b[2] and a[3] == b[3] and a[3] < 43
    assert a[0] == b[0]
    # the occupancy refreshes evaluated the same densities through the selected copy (cells drawn twice in one refresh keep either of their two
    # jittered evaluations -- "any of them wins", as in the reference -- so the mean may move in its last digits from run to run)
    np.testing.assert_allclose(a[6], b[6], rtol=1e-5, atol=0)
    assert torch.equal(a[4], b[4])
    for x, y in zip(a[5], b[5]):
        assert torch.equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[7], b[7])
    assert a[8] == b[8]


# ---------------------------------------------------------------------------------------------------------------------------------
# The table seen from outside the graphs, at every parity.  Reference: the same schedule with fused_table_adam=False (the
# separate k_adam sweep: one buffer set, no parity); every comparison is torch.equal -- the two modes are the same training bit for bit
# (test_graphed_training_with_fused_table_adam_is_the_same_training), so nothing here has a tolerance.
# ---------------------------------------------------------------------------------------------------------------------------------
N_RAYS = 1024
KW = dict(staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
# 2^7: with it every step of these schedules STANDS (asserted from the step count scalars[3] wherever a parity is claimed; the default 2^16
# would overflow and skip a few first steps, and a skipped step does not flip)
STANDING_SCALE = 128.0


class _Run:
    """one training run under GraphedTrainStep: 16 eager steps (the sample estimate does not exist before the first occupancy refresh),
    then captured ones; `steps(k)` -> how many of the k stood"""

    def __init__(self, dev, fuse, lookahead, encoder=None, **st_kw):
        from graph import GraphedTrainStep
        from optim import NGPEma
        occ = torch.from_numpy(sc.occupancy_density()).to(dev)
        bits = torch.from_numpy(oracle.packbits(sc.occupancy_density(), 10.0)).to(dev)
        self.batches = []
        for i in range(48):
            o, d, gt = sc.training_batch(N_RAYS, seed=300 + i)
            self.batches.append((torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)))

        def keep(m):
            m.density_bitfield.copy_(bits)
            m.density_grid.copy_(occ)
        self.model, self.opt = _make_ngp(dev, encoder)
        self.opt.scalars[0] = STANDING_SCALE
        self.fuse, self.lookahead = fuse, lookahead
        self.st = GraphedTrainStep(self.model, self.opt, None, N_RAYS, KW, after_update=keep, direct=True, lookahead=lookahead,
                                   fused_table_adam=fuse, **st_kw)
        self.emb = self.model.encoder.embeddings
        self.i, self.losses, self.problems = 0, [], []
        assert self.steps(16) == 16 and self.st.n_captures == 0          # eager so far, nothing skipped
        self.ema = NGPEma([p for p in self.model.parameters() if p.requires_grad], 0.95, optimizer=self.opt)
        self.pts = torch.rand(4096, 3, device=dev, generator=torch.Generator(device='cuda').manual_seed(11)) * 2 - 1

    def count(self):
        return float(self.opt.scalars[3])

    def steps(self, k):
        before, n = self.count(), len(self.batches)
        for _ in range(k):
            nxt = dict(next_rays=self.batches[(self.i + 1) % n]) if self.lookahead else {}
            self.losses.append(float(self.st.step(*self.batches[self.i % n], **nxt)))
            self.i += 1
        return int(self.count() - before)

    def captured(self, fused=None):
        st = self.st
        assert st.capture_error is None and st.n_captures >= 1 and st.used_direct and st.graphs is not None
        assert st.table_fused == (self.fuse if fused is None else fused)

    def after_observation(self, tag):
        """whoever looked has made buffer set A the current one"""
        if float(self.opt.scalars[5]) != 0.0:
            self.problems.append(f'{tag}: the parity word is {float(self.opt.scalars[5])} after the observation')
        if not torch.equal(self.emb._ngp_fp16, self.emb.detach().half()):
            self.problems.append(f'{tag}: the fp16 shadow of the Parameter is not the Parameter in fp16')

    def close(self):
        self.st.close()


def _table_state(run):
    run.st.sync_params()
    st, m = run.opt.state[run.emb], run.model
    out = dict(emb=run.emb, exp_avg=st['exp_avg'], exp_avg_sq=st['exp_avg_sq'], fp16=run.emb._ngp_fp16, sigma=m.sigma_net.weights,
               color=m.color_net.weights, sigma_m=run.opt.state[m.sigma_net.weights]['exp_avg'], scalars=run.opt.scalars[:5])
    return {k: v.detach().clone() for k, v in out.items()}


def _read_checkpoint(run):
    import checkpoint
    state = checkpoint.save_checkpoint('unwritten', run.model, optimizer=run.opt, full=True, write=False)
    return dict(emb=state['model']['encoder.embeddings'].detach().clone())   # (state_dict() hands out the live tensors: copy now)


def _read_state_dict(run):
    sd = run.opt.state_dict()
    out = {f'exp_avg{i}': t for i, t in enumerate(sd['exp_avg'])}
    out.update({f'exp_avg_sq{i}': t for i, t in enumerate(sd['exp_avg_sq'])})
    return out


def _read_ema(run):
    e = run.ema
    e.update()
    e.store()
    e.copy_to()
    e.restore()
    out = {f'shadow{i}': t.detach().clone() for i, t in enumerate(e.shadow_params)}
    out.update({f'restored{i}': p.detach().clone() for i, p in enumerate(e.params)})
    return out


def _read_frame(run):
    b, m = run.batches[0], run.model
    m.eval()
    try:
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
            return dict(frame=m.render(b[0], b[1], staged=False, bg_color=1, perturb=False, max_steps=1024)['image'].detach().clone())
    finally:
        m.train()


def _read_encoder(run):
    with torch.no_grad():
        return dict(encoded=run.model.encoder(run.pts, bound=1).detach().clone())


READERS = (('save_checkpoint', _read_checkpoint), ('state_dict', _read_state_dict), ('sync_params', _table_state), ('ema', _read_ema),
           ('eval frame', _read_frame), ('drop-in encoder', _read_encoder))


def _differences(tag, a, b):
    """names of what differs between two observations (dicts of tensors) of the fused run `a` and the separately swept run `b`"""
    assert a.keys() == b.keys()
    return [f'{tag}: {k} differs from the unfused run (max |diff| {float((a[k].double() - b[k].double()).abs().max()):.3g})'
            for k in a if not torch.equal(a[k], b[k])]


# standing steps between two observations.  Every observation leaves parity 0 behind, so an observation after an odd count meets buffer set B
# as the current one, after an even count set A.  (The first five are the parities 1, 0, 0, 1, 0 of a word nobody resets; the rest gives every
# reader an odd and an even count.)
K_SEQ = (1, 1, 2, 3, 1, 2, 4, 2, 1, 2, 3, 2)


@pytest.mark.parametrize('lookahead', [True, False])
def test_readers_outside_the_graphs_see_the_current_table_at_every_parity(lookahead):
    """every reader after odd and after even numbers of standing replays.  materialize() is gated on a host flag that Python sets when it
    issues a fused step, i.e. at capture time; the stepper states every replay (optim.replayed_fused_table_step).  Without that statement
    only the first observation finds the flag set: a later one after an odd count returns buffer set A, one step stale, and leaves the
    parity word at 1 -- which is what the assertions after each observation and the comparison with the unfused run look for."""
    dev = torch.device('cuda')
    odd, even = [j for j, k in enumerate(K_SEQ) if k % 2], [j for j, k in enumerate(K_SEQ) if not k % 2]
    assert len(odd) == len(even) == len(READERS)
    shift = 0 if lookahead else 3          # (the two cases also differ in who comes first, while the capture-time flag still holds)
    reader_at = {}
    for i, (jo, je) in enumerate(zip(odd, even)):
        reader_at[jo] = reader_at[je] = READERS[(i + shift) % len(READERS)]
    seen, runs = {}, {}
    for fuse in (True, False):
        run = _Run(dev, fuse, lookahead)
        obs = []
        for j, k in enumerate(K_SEQ):
            assert run.steps(k) == k, (j, k)              # all of them stood: k flips since the last observation
            name, read = reader_at[j]
            tag = f'observation {j} ({name}) after {k} standing step(s)'
            obs.append((tag, read(run)))
            run.after_observation(tag)
            seen.setdefault(name, set()).add(k % 2)
        run.captured()
        runs[fuse] = (obs, run.losses, run.problems)
        run.close()
    assert all(v == {0, 1} for v in seen.values()) and len(seen) == len(READERS)
    problems = runs[True][2] + runs[False][2]
    for (tag, a), (_, b) in zip(runs[True][0], runs[False][0]):
        problems += _differences(tag, a, b)
    assert not problems, '\n'.join(problems)
    assert runs[True][1] == runs[False][1]


@pytest.mark.parametrize('lookahead', [True, False])
def test_skipped_steps_do_not_count_as_flips(lookahead):
    """stretches that start from an overflowing loss scale (an ordinary GradScaler skip: the scale halves until a step stands): what decides
    which buffer set is current is the number of steps that STOOD, not the number replayed -- the schedule goes on until it has observed after
    (even replayed, odd standing) and after (odd replayed, even standing)."""
    dev = torch.device('cuda')
    runs = {}
    for fuse in (True, False):
        run = _Run(dev, fuse, lookahead)
        assert run.steps(1) == 1
        run.captured()
        first = _table_state(run)
        run.after_observation('first')
        obs, counts, combos = [('first', first)], [], set()
        for attempt in range(9):
            if {(0, 1), (1, 0)} <= combos:
                break
            want = 1 + attempt % 2                          # standing steps of this stretch
            # 2^32, 2^33, 2^34 (the image gradient alone, ~1e-4, leaves the fp16 range): the number of skipped steps moves by one
            run.opt.scalars[0] = 2.0 ** (32 + attempt % 3)
            replayed = 0
            while want:
                want -= run.steps(1)
                replayed += 1
                assert replayed < 60
            standing = 1 + attempt % 2
            assert replayed > standing                      # something was skipped
            combos.add((replayed % 2, standing % 2))
            counts.append((replayed, standing))
            name, read = READERS[0] if attempt % 2 == 0 else READERS[2]
            tag = f'stretch {attempt} ({name}): {replayed} replayed, {standing} standing'
            obs.append((tag, read(run)))
            run.after_observation(tag)
        assert {(0, 1), (1, 0)} <= combos, counts
        runs[fuse] = (obs, run.losses, run.problems, counts)
        run.close()
    assert runs[True][3] == runs[False][3]
    problems = runs[True][2] + runs[False][2]
    for (tag, a), (_, b) in zip(runs[True][0], runs[False][0]):
        problems += _differences(tag, a, b)
    assert not problems, '\n'.join(problems)
    assert np.array_equal(runs[True][1], runs[False][1], equal_nan=True)


def _drop_in_step(run):
    """one iteration through the drop-in path (autograd) and an UNFUSED optimizer step"""
    b = run.batches[40]
    with torch.autocast('cuda', dtype=torch.float16):
        out = run.model.render(b[0], b[1], **KW)
        loss = ((out['image'] - b[2]) ** 2).mean()
    run.opt.scale(loss).backward()
    run.opt.step()
    run.losses.append(float(loss.detach()))


@pytest.mark.parametrize('lookahead', [True, False])
def test_writers_outside_the_graphs_write_the_current_table(lookahead, tmp_path):
    """an unfused step, a checkpoint load (model only / full) and the EMA weights of an evaluation, each after an ODD number of standing
    replays (buffer set B current): what they write must be what the next replays train on -- written into buffer set A while the graphs go
    on with B, the eager update, the loaded table and the EMA weights would be lost."""
    import checkpoint
    dev = torch.device('cuda')
    runs = {}
    for fuse in (True, False):
        run = _Run(dev, fuse, lookahead)
        obs = []

        def observe(tag):
            obs.append((tag, _table_state(run)))
            run.after_observation(tag)
            obs.append((tag + ' [losses]', dict(losses=torch.tensor(run.losses, dtype=torch.float64))))
        assert run.steps(1) == 1
        run.captured()
        path = str(tmp_path / f'ck_{fuse}.pth')
        checkpoint.save_checkpoint(path, run.model, optimizer=run.opt, full=True)   # (the first reader: the capture-time flag still holds)
        run.after_observation('save')
        # -- an unfused step
        assert run.steps(1) == 1
        _drop_in_step(run)
        assert run.steps(1) == 1
        observe('1 replay after the unfused step')
        assert run.steps(3) == 3
        observe('3 more replays after the unfused step')
        # -- a model-only load: the loaded table is what the next step renders
        assert run.steps(1) == 1
        checkpoint.load_checkpoint(path, run.model, optimizer=run.opt, model_only=True)
        assert run.steps(2) == 2
        observe('2 replays after load_checkpoint(model_only=True)')
        # -- a full load (NGPAdam.load_state_dict: moments, step count, loss scale as well)
        assert run.steps(3) == 3
        checkpoint.load_checkpoint(path, run.model, optimizer=run.opt)
        assert run.steps(2) == 2
        observe('2 replays after the full load_checkpoint')
        # -- the EMA weights around an evaluation, with a training step in between
        assert run.steps(1) == 1
        run.ema.update()
        run.after_observation('ema.update')
        assert run.steps(1) == 1
        run.ema.store()
        run.ema.copy_to()
        assert run.steps(1) == 1
        observe('1 replay on the EMA weights')
        assert run.steps(1) == 1
        run.ema.restore()
        assert run.steps(2) == 2
        observe('2 replays after ema.restore')
        run.captured()
        runs[fuse] = (obs, run.problems)
        run.close()
    problems = runs[True][1] + runs[False][1]
    for (tag, a), (_, b) in zip(runs[True][0], runs[False][0]):
        problems += _differences(tag, a, b)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('lookahead', [True, False])
def test_capacity_switch_and_recapture_at_odd_parity(lookahead):
    """the capacity ladder: `_activate` switches between captured graphs without running Python's iteration, a re-capture starts from buffer
    set A (`_capture` -> sync_params).  Both with an odd number of standing steps behind them."""
    dev = torch.device('cuda')
    runs = {}
    for fuse in (True, False):
        run = _Run(dev, fuse, lookahead, capacity_ladder=(1.25,))
        st, m = run.st, run.model
        obs = []
        assert run.steps(1) == 1
        run.captured()
        base = st.captured_capacity
        assert st.precapture(update_modes=()) == 1 and st.captured_capacity == base and st.n_captures == 2
        rung, switches = max(st._captured), st.n_switches
        assert rung > base and getattr(st, 'ladder_error', None) is None
        obs.append(('after the capture', _table_state(run)))
        run.after_observation('after the capture')
        # a switch: one standing step on the base graphs, then the estimate moves into the rung's window
        assert run.steps(1) == 1
        m.mean_count = rung - 128 - st.quantum // 2
        assert run.steps(2) == 2
        assert st.n_switches == switches + 1 and st.captured_capacity == rung and st.n_captures == 2
        run.captured()
        obs.append(('3 standing steps, a switch after the first', _read_checkpoint(run)))
        run.after_observation('switch')
        # a re-capture: one standing step, then an estimate no captured capacity serves
        assert run.steps(1) == 1
        m.mean_count = 2 * rung
        assert run.steps(1) == 1
        assert st.n_captures == 3 and st.captured_capacity > rung
        run.captured()
        obs.append(('1 standing step after a re-capture behind 1 standing step', _table_state(run)))
        run.after_observation('re-capture')
        assert run.steps(2) == 2
        obs.append(('2 more', _read_state_dict(run)))
        run.after_observation('2 more')
        assert run.i < 32                                   # (no occupancy refresh in between: the estimate stayed where the test put it)
        runs[fuse] = (obs, run.losses, run.problems)
        run.close()
    problems = runs[True][2] + runs[False][2]
    for (tag, a), (_, b) in zip(runs[True][0], runs[False][0]):
        problems += _differences(tag, a, b)
    assert not problems, '\n'.join(problems)
    assert runs[True][1] == runs[False][1]


# 16 levels x 2 features on the lego batch.  A dense level rides in the prefix that the closing launch sweeps while it has <= 128 x 4096
# entries (plan_backward's round-robin bins), so the hash-table size does not fill the prefix: with the flagship geometry (16 -> 2048) it is
# 352 696 entries for log2_hashmap_size <= 19, and from 20 on level 5 (83^3 = 551 368 entries, dense) is too large for those bins and the grid
# backward cannot carry the sweep at all (the query says 0xffffffff) -- no log2_hashmap_size reaches the 4 M cap of
# ngp_optim_adam_small_commit.  A slowly growing grid does: 32 -> 96 has 13 dense levels, 2 357 584 entries = 4 715 168 parameters.
UNFUSABLE_GRIDS = [
    (dict(base_resolution=16, log2_hashmap_size=20, desired_resolution=2048), 0xffffffff),
    (dict(base_resolution=32, log2_hashmap_size=19, desired_resolution=96), 2357584),
]


@pytest.mark.parametrize('encoder,prefix', UNFUSABLE_GRIDS, ids=['dense level beyond the bins', 'prefix beyond the cap'])
def test_a_table_the_closing_launch_cannot_serve_is_graphed_with_the_separate_sweep(encoder, prefix):
    """fusion is decided before enable_table_fusion (graph._table_fusion_fits -> optim.table_fusion_fits): enabled for such a table, the
    capture of the step fails, becomes capture_error, and the run stays eager for good without saying so"""
    import _ngp_capi as capi
    import optim
    dev = torch.device('cuda')
    run = _Run(dev, True, True, encoder=encoder)
    assert run.st.fused_table_adam
    assert run.steps(3) == 3
    st, enc = run.st, run.model.encoder
    arr = capi.host_offsets(enc.offsets)
    got = int(capi.lib.ngp_grid_table_adam_prefix(ctypes.cast(arr, ctypes.c_void_p), st.captured_capacity, 3, 2, 16, float(np.log2(enc.per_level_scale)),
                                                  enc.base_resolution, enc.gridtype_id, 0, capi.NGP_F16))
    assert got == prefix
    rest = run.model.sigma_net.weights.numel() + run.model.color_net.weights.numel()
    assert prefix == 0xffffffff or prefix * 2 + rest > optim.SMALL_COMMIT_MAX_PARAMS
    assert st.table_fused is False and st.capture_error is None and st.n_captures >= 1
    assert st.graphs is not None and st.used_direct and run.opt.fused_table is None
    assert all(np.isfinite(run.losses))
    run.close()
