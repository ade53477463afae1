"""HIP-graph replay of the training iteration (MI355X-native replacement for ~80 eager launches per step).

One `--fp16 --cuda_ray --ff` iteration is ~80 kernel launches of 2-500 us each; issued eagerly the host needs longer to
enqueue them than the GPU needs to run them.  `GraphedTrainStep` captures

    optimizer.zero_grad -> model.render (near/far, march, fused sample pipeline, composite) -> loss -> scaled backward
    [-> gradient all-reduce, eager, between two graphs when world_size > 1] -> GradScaler.step(fused Adam) -> GradScaler.update

into HIP graphs (`torch.cuda.CUDAGraph`; every kernel of libngp_hip.so is launched on the capturing stream through the C
ABI, so it is captured like any PyTorch kernel) and replays them per step.  Everything the iteration needs is
device-resident: the sample buffer is sized from the running `mean_count` estimate (no host read-back, rays that do not fit
are dropped whole exactly as in the reference, raymarching.cu:405-416), GradScaler's inf check feeds the fused Adam
kernel as a tensor, and the only per-step host work is three small device copies (the batch into the static input buffers)
and one graph launch.

What stays eager, at the reference Trainer's cadence (nerf/utils.py:851-856): `update_extra_state` every 16 steps, which also
refreshes `mean_count`.  The captured sample capacity is `mean_count` rounded up to a multiple of `capacity_quantum`
(default 8192 samples, ~3 % of a lego-sized batch) and is kept while the estimate stays inside [capacity - 2 quanta, capacity]
(a larger buffer only drops fewer rays than the reference's `mean_count`-sized one), so the graph is re-captured only when the
estimate grows past the captured buffer or falls well below it.  `precapture()` records every graph a steady-state run replays
(the iteration and the occupancy refresh) up front, so that no one-time capture cost lands inside a measured or latency-critical
stretch of steps.

`lookahead=True` (single rank, autograd-free iteration): `step(rays_o, rays_d, target, next_rays=(o, d))` also marches the NEXT batch
-- near/far + march_rays_train need no weights -- on a side stream while this iteration's encode .. Adam run.  The marcher is latency-bound
(one wavefront per ray, ~60 us with the chip mostly idle), so about half of it disappears under the rest of the step.  Two sample-buffer
sets alternate; per set one march graph and one "rest" graph (separate memory pools: they replay concurrently).  Same arithmetic in
the same order per batch; only the in-kernel start offsets of `perturb=True` are seeded by the step index instead of the optimizer's
step count (the two agree unless a step was skipped).  The step before an occupancy refresh does not look ahead: the refreshed bitfield
must be marched.

Command lists (autograd-free iteration with `optim.NGPAdam`, single GPU; `_cmdlist_ok`): the rest graph's chain consists of the library's own
launches, so it is also recorded into a native command list (cmdlist.py, csrc/cmdlist.cpp) while it is captured, and a step replays the
list -- the same launches with the same arguments issued from C, 6-7 us per step less idle GPU at the step boundary than the graph launch
(DESIGN.md section 4).  The graph is kept: it owns the buffers the list points into and serves every configuration that is not eligible.
NGP_STEP_CMDLIST=0 keeps the graph replay; NGP_STEP_MARCH_AT moves the start of the lookahead march to a mark inside the chain (measured:
slower everywhere but at the step boundary, the default).

Requirements: a torch optimizer constructed with `capturable=True` (and preferably `fused=True`) plus a GradScaler, or
`optim.NGPAdam` with `scaler=None` (it owns the loss scale; `averager` may then be the optimizer itself); the model has completed at least
one `update_extra_state` after 16 eager steps (`model.mean_count > 0`) -- before that the sample buffer is sized for the
worst case and read back, which cannot be captured, and `step()` simply runs eagerly.
"""
import contextlib
import dataclasses
import operator
import os
import typing
from collections import namedtuple

import torch


def _capture_into(g, **kw):
    """torch.cuda.graph(g, ...).  With a torch.distributed process group alive its watchdog thread polls HIP events while this thread
    captures; in the default 'global' capture mode such a call from ANOTHER thread invalidates the capture -- 'thread_local' restricts the
    check to the capturing thread (the data-parallel path captures three graphs around its collectives)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        kw.setdefault('capture_error_mode', 'thread_local')
    return torch.cuda.graph(g, **kw)


# NGP_STEP_MARCH_AT: where in the main chain the side stream may begin the next batch's march (lookahead steps replayed from a command
# list): the step boundary (what the graph replay does), or a mark at (kernel name, 1: behind that launch / 0: in front of it) --
# behind the network forward, behind the compositor, behind the sigma backward (= where the record sort starts), behind the sort
MARCH_MARKS = {'boundary': None, 'net': ('k_network_forward', 1), 'composite': ('k_composite_train', 1), 'sigma': ('k_grid_backward_bin', 0),
               'sort': ('k_grid_backward_accumulate', 0)}
MARCH_MARK_ID = 1


# one of the lookahead's two buffer sets as one capture recorded it: the march graph (static rays of the set -> its samples; replays on the
# side stream), the rest graph (samples + target -> loss, gradients, optimizer step), the static loss and [N,3] image buffers the rest chain
# writes, and the two closures of fused_train_iteration_split (they keep the marched buffers alive)
_LaSet = namedtuple('_LaSet', 'march_graph rest_graph loss image march rest', defaults=(None, None))

# the occupancy refresh as graphs: `graph` -> `mean`, the device mean density.  The split form (lookahead) carries the cell sampling as a graph
# of its own (`sampling` -> `samples`), which may replay on the side stream under the previous iteration; the whole form has both None
_Refresh = namedtuple('_Refresh', 'graph mean sampling samples', defaults=(None, None))

# what a stepper that is collected inside ANOTHER stepper's stream capture keeps alive until a synchronize is allowed again
_Parked = namedtuple('_Parked', 'active captured update_graphs side optimizer sample_pool')


@dataclasses.dataclass(eq=False, slots=True)
class _Capture:
    """everything ONE capture produced and decided, for one sample capacity: `GraphedTrainStep._captured` is {capacity: _Capture}, the
    stepper steps through `active`.  A field that is not stated here does not exist -- nothing of a capture lives on the stepper, where a
    switch to another capacity would leave it behind."""
    capacity: typing.Optional[int] = None   # None: nothing is captured (before the first capture, after a failed one)
    # one step of this capture's replay shape: replay(stepper, rays_o, rays_d, target, next_rays) -> the device loss.  The plain function,
    # not a bound method: a record that owned its stepper would leave the stepper's close() to the cyclic collector
    replay: typing.Any = None
    graphs: typing.Any = None        # every training graph, in capture order
    # the rest graphs' launch chains as native command lists (cmdlist.CommandList, one per rest graph; None: the graphs are replayed)
    lists: typing.Any = None
    loss: typing.Any = None          # the static loss (single buffer set) ...
    image: typing.Any = None         # ... and image buffer
    la: typing.Any = None            # [_LaSet] x 2: the lookahead shape
    la_apply: typing.Any = None      # sharded lookahead with eager collectives: the graph of the shard update
    rest_pool: typing.Any = None     # the lookahead's rest graphs' memory pool (the refresh's density half joins it)
    sharded: bool = False            # the three graphs around the two collectives
    used_direct: bool = False        # the autograd-free iteration was captured
    table_fused: bool = False        # the table's Adam sweep rides in the grid backward (needs the producers' non-finite sweep)
    producers_check: bool = False    # the producers flag non-finite gradients: the optimizer step skips its own sweep
    checked_ok: bool = False         # they could (fused.iteration_checks_gradients)

    def get(self, field):
        """a field by name, as readers of `_captured`'s values spell it (tests/test_gpu_step_cmdlist.py: `snap.get('lists')`); strict: a
        name that is no field raises AttributeError, there is no default to hide behind"""
        return getattr(self, field)


class _Announced(namedtuple('_Announced', 'rays_o rays_d ray_versions epoch target target_version', defaults=(None, None))):
    """a batch that was staged ahead of its step (marched into a lookahead buffer set, or copied into the sharded step's static buffers).
    Holds REFERENCES to the announced tensors, compared by identity plus `_version`: a freed tensor's address can be handed out again by
    the caching allocator (same data_ptr, fresh _version 0), which an address/version key would take for a hit.
    target None: the rays were announced without it.  epoch: the occupancy epoch a march saw (None: the staging does not depend on the grid)"""
    __slots__ = ()

    @classmethod
    def of(cls, rays_o, rays_d, target=None, epoch=None):
        return cls(rays_o, rays_d, (rays_o._version, rays_d._version), epoch, target, None if target is None else target._version)

    def holds_rays(self, rays_o, rays_d, epoch=None):
        return self.rays_o is rays_o and self.rays_d is rays_d and self.ray_versions == (rays_o._version, rays_d._version) and self.epoch == epoch

    def holds_target(self, target):
        return self.target is target and self.target_version == target._version


_PARKED = []   # _Parked of steppers that were collected while another stepper was capturing (GraphedTrainStep.close), evicted _Capture


def _drain_parked():
    """release what close() had to park; called outside any capture (the start of a capture, an ordinary close())"""
    if _PARKED and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize()
        del _PARKED[:]


def mse_loss(out, target):
    # mean over rays and channels of the squared error (nerf/utils.py:516,557) through PyTorch's fused MSE kernels
    return torch.nn.functional.mse_loss(out['image'][0], target)


class GraphedTrainStep:
    def __init__(self, model, optimizer, scaler, n_rays, render_kwargs, loss_fn=mse_loss, averager=None, capacity_quantum=8192,
                 update_interval=16, after_update=None, autocast_dtype=torch.float16, direct=True, capacity_slack=2, lookahead=False,
                 fused_table_adam=False, capacity_ladder=(0.8, 1.25, 1.5625, 1.953125, 2.44140625), geo_loss=None):
        """geo_loss: a fused.GeoLoss(lambda_distortion=...) -- the autograd-free iteration adds the distortion term to the MSE loss inside its
        compositor launch (fused.fused_train_iteration(geo_loss=)), in the single buffer set and the lookahead sets, captured
        or not; the eager steps before the first capture render with geo=True and add the same term through autograd.  Needs the direct
        iteration: a configuration or a model that is not eligible for it raises instead of training without the term (an arbitrary loss_fn
        cannot be asked to add it).  The lambda is a host float baked into the captured launches: another value needs a new GraphedTrainStep.
        lambda_depth > 0 is refused (ValueError): depth targets are per-batch tensors the static and lookahead buffer sets do not hold yet --
        use the eager fused.fused_train_iteration for depth supervision."""
        self.model, self.optimizer, self.scaler = model, optimizer, scaler
        self.loss_fn, self.averager = loss_fn, averager
        if averager is not None and averager is not optimizer and getattr(optimizer, 'flat_grad16', None) is not None:
            # a gradient-depositing optimizer keeps the table gradient in its own fp16 buffer (p.grad stays None): only its own
            # all_reduce() sees it -- a foreign averager would average nothing and make the optimizer step on zeros
            raise RuntimeError('GraphedTrainStep: with optim.NGPAdam(deposit=True) pass the optimizer itself as `averager`')
        self.render_kwargs = dict(render_kwargs)
        self.quantum = int(capacity_quantum)
        self.slack = int(capacity_slack)  # quanta the estimate may fall below the captured capacity before a re-capture
        self.update_interval = int(update_interval)
        self.after_update = after_update
        self.autocast_dtype = autocast_dtype
        dev = next(model.parameters()).device
        self.dev = dev
        self.rays_o = torch.zeros(1, n_rays, 3, device=dev)
        self.rays_d = torch.zeros(1, n_rays, 3, device=dev)
        self.target = torch.zeros(n_rays, 3, device=dev)
        self.counter = torch.zeros(16, 2, dtype=torch.int32, device=dev)  # row 0 is the captured marcher's counter
        self.global_step = 0
        self.captured_capacity = None
        # every capacity captured so far: {capacity: the graphs and what belongs to them}.  A sample estimate that leaves the active buffer's
        # window first looks for another captured capacity that serves it (a switch costs nothing) before anything is captured anew;
        # `precapture()` records a LADDER of capacities (this one x capacity_ladder) up front, so that a training run whose occupancy grid
        # follows the density network -- the estimate moves by tens of percent over the first thousands of steps (renderer.py:531-538) --
        # does not stop to capture (round 5: two re-captures in 96 steps made that stretch run at 1.98 ms / step against 0.43)
        self._captured = {}
        self.active = _Capture()    # the record this stepper replays (and, during a capture, the one being filled in)
        self.capacity_ladder = tuple(float(f) for f in (capacity_ladder or ()))
        self.ladder_error = None    # a rung of the ladder that could not be captured (the rungs before it are kept)
        self.n_switches = 0
        # command lists replace the replay of the rest graphs where the step is eligible.  NGP_STEP_CMDLIST=0: keep the graph replay in this build
        self.use_lists = os.environ.get('NGP_STEP_CMDLIST', '1') != '0'
        self.march_at = os.environ.get('NGP_STEP_MARCH_AT', 'boundary')
        if self.march_at not in MARCH_MARKS:
            raise ValueError(f'NGP_STEP_MARCH_AT={self.march_at!r}: one of {sorted(MARCH_MARKS)}')
        self.n_list_replays = 0
        # the finished [N,3] fp32 image of the step that ran last: a view of a static buffer of the captured step (or the eager step's
        # render), valid until the next step() -- what an error-map update needs besides the loss (nerf.utils.ErrorMaps)
        self.image = None
        self.n_captures = 0
        self.capture_error = None
        self.graph_updates = True   # replay the occupancy refresh from a HIP graph as well (see _update_extra_state)
        self.update_graphs = {}     # {full sweep?: _Refresh}
        self._sample_pool = None    # memory pool of the refresh's sampling graphs (they replay on the side stream)
        self.n_update_captures = 0
        self.update_capture_error = None
        self.capacity = None  # sample capacity of the step that ran last (None while eager/worst-case)
        # autograd-free iteration (fused.fused_train_iteration): needs the default loss, an optimizer that owns its loss scale and
        # deposits gradients (optim.NGPAdam), and a model/render configuration the fused training render accepts
        self.direct = bool(direct) and loss_fn is mse_loss and scaler is None and getattr(optimizer, 'flat_grad16', None) is not None
        # lookahead: the next batch's march under this iteration (see the module docstring); single rank + autograd-free iteration only
        self.geo_loss = geo_loss
        if geo_loss is not None:
            from fused import GeoLoss
            if not isinstance(geo_loss, GeoLoss):
                raise TypeError('GraphedTrainStep: geo_loss must be a fused.GeoLoss')
            if geo_loss.lambda_depth > 0:
                raise ValueError('GraphedTrainStep: lambda_depth > 0 is not supported under the graphs (depth targets are per-batch tensors); '
                                 'use fused.fused_train_iteration(geo_loss=) eagerly')
            if not self.direct or self.render_kwargs.get('geo', False) or self.render_kwargs.get('staged', False):
                raise ValueError('GraphedTrainStep: geo_loss needs the autograd-free iteration (direct=True, the default loss_fn, scaler=None, '
                                 "optim.NGPAdam) and render_kwargs without 'geo' / 'staged'")
        # the sharded data-parallel update: optim.NGPAdam(shard=True) that is its own averager (it exchanges the flat gradient buffer itself)
        self.shards = averager is optimizer and bool(getattr(optimizer, 'shard', False))
        self.lookahead = bool(lookahead) and self.direct and (averager is None or self.shards)
        self.la_cur = 0                     # buffer set of the CURRENT batch
        self.la_ready = [None, None]        # what is marched into each set (_Announced; None: nothing)
        self.la_hits = 0                    # steps whose march had been done ahead
        self._precopied = None              # sharded step: the batch already copied into the static buffers (_Announced)
        self.occupancy_epoch = 0
        self.la_presampled = None           # refresh mode (full sweep?) whose cell sampling already ran on the side stream
        self.la_presample_hits = 0
        # sharded lookahead only: capture the two RCCL collectives INSIDE the rest graph (one replay per step on the main stream) instead of
        # issuing them eagerly between two replays.  Off by default: measurable here only over a 1-rank group (bench.py ddp_overhead_1rank)
        self.graph_collectives = os.environ.get('NGP_GRAPH_COLLECTIVES', '0') == '1'
        # single GPU, autograd-free iteration, optim.NGPAdam: the hash table's Adam sweep rides in the grid backward's slice accumulate
        # (speculative double buffer, parity flipped by the commit: optim.NGPAdam.enable_table_fusion) -- k_adam over 12 M parameters and the
        # scale update become one small launch.  The torch Parameter is then one of two buffer sets: read it through `sync_params()`.
        self.fused_table_adam = bool(fused_table_adam) and self.direct and averager is None and hasattr(optimizer, 'enable_table_fusion')
        self.la_side = None
        if self.lookahead:
            self.la_rays_o = [torch.zeros(n_rays, 3, device=dev) for _ in range(2)]
            self.la_rays_d = [torch.zeros(n_rays, 3, device=dev) for _ in range(2)]
            self.la_target = [torch.zeros(n_rays, 3, device=dev) for _ in range(2)]
            self.la_seed = torch.zeros(2, dtype=torch.int32, device=dev)
            self.la_side = torch.cuda.Stream(device=dev)
            self.la_event = [torch.cuda.Event(), torch.cuda.Event()]
            self.la_sample_event = torch.cuda.Event()
            self.la_slot_event = None   # recorded on the main stream behind its latest write to the model's sample-count ring (a lookahead miss)

    # ------------------------------------------------------------------------------------------
    def close(self):
        """wait for everything this object queued -- including the side stream's march of a batch that will never be consumed (the last
        step announces its successor) -- BEFORE its graphs and their private memory pools are released.  Round 4 suspected that a HIP graph
        destroyed while one of its replays is still running hands its pool back to the allocator under the running kernels; round 5 made
        the situation deterministic (tests/test_gpu_graph_lifetime.py, tools/graph_lifetime_probe.py: side stream held by a spin kernel) and
        found that the graph destruction ITSELF waits for the replay on this runtime -- no use-after-free with or without this method.  It
        stays as the explicit statement of the ordering (and for runtimes that do not wait).  Called by __del__."""
        # __del__ runs this on an object whose __init__ raised half-way as well: the ONE place where the stepper's own fields are read with
        # getattr defaults
        side, active, captured = getattr(self, 'la_side', None), getattr(self, 'active', _Capture()), getattr(self, '_captured', {})
        update_graphs = getattr(self, 'update_graphs', None)
        try:
            # this object may be collected by the cyclic GC while ANOTHER stepper is inside a stream capture: a synchronize (or
            # any stream / event query) there would invalidate that capture.  The graphs and everything they replay into are parked instead
            # and released by the next close() / capture that runs outside a capture (_drain_parked)
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                _PARKED.append(_Parked(active, captured, update_graphs, side, getattr(self, 'optimizer', None), getattr(self, '_sample_pool', None)))
                return
            if side is not None:
                side.synchronize()
            comm = getattr(getattr(self, 'optimizer', None), '_comm_stream', None)
            if comm is not None:
                comm.synchronize()
            if torch.cuda.is_available() and (active.graphs is not None or update_graphs):
                torch.cuda.current_stream().synchronize()
            # the lists go before the graphs that own their buffers (this object steps through the graphs from here on)
            for rec in [active, *captured.values()]:
                for cl in rec.lists or ():
                    cl.destroy()
                rec.lists = None
            _drain_parked()
        except Exception:  # noqa: BLE001 -- interpreter shutdown: the device context may be gone already
            pass

    def __del__(self):
        self.close()

    def _capacity(self):
        mc = int(self.model.mean_count)
        if mc <= 0:
            return None
        return ((mc + 128 + self.quantum - 1) // self.quantum) * self.quantum

    # what the active capture holds, readable on the stepper (read-only: a capture is changed through its record)
    graphs, lists, loss, la, la_apply, sharded, used_direct, table_fused, producers_check, _checked_ok = (
        property(operator.attrgetter('active.' + field)) for field in
        ('graphs', 'lists', 'loss', 'la', 'la_apply', 'sharded', 'used_direct', 'table_fused', 'producers_check', 'checked_ok'))

    def _activate(self, cap):
        """make the graphs captured for `cap` samples the active ones (no device work).  A batch the side stream marched ahead sits in the
        OLD capacity's buffers: it is forgotten (the next step marches its batch in line) -- a switch follows an occupancy refresh, and the
        step before a refresh does not look ahead anyway."""
        self.active = self._captured[cap]
        if cap != self.captured_capacity:
            self.n_switches += 1
        self.captured_capacity = cap
        self.la_ready = [None, None]

    def _pick_captured(self, cap):
        """the smallest captured capacity that holds an estimate of `cap` samples without wasting more than ~30 % of its rows (None: capture)"""
        fits = [c for c in self._captured if c >= cap and c <= cap * 1.3 + self.slack * self.quantum]
        return min(fits) if fits else None

    def _fits(self, cap):
        """the captured buffer still serves an estimate of `cap` samples (hysteresis: see the module docstring)"""
        return (self.graphs is not None and self.captured_capacity is not None
                and self.captured_capacity - self.slack * self.quantum <= cap <= self.captured_capacity)

    @property
    def captures(self):
        """number of graph captures so far (training iteration + occupancy refresh); constant over a stretch of steps = pure replay"""
        return self.n_captures + self.n_update_captures

    def precapture(self, update_modes=None):
        """capture, without executing anything, every graph the coming steps will replay: the training iteration (needs the
        `mean_count` estimate, i.e. >= 16 eager steps and one update_extra_state) and the occupancy refresh in the given modes
        (True = full sweep, False = partial; default: the mode the model is in now and, while it still does full sweeps, the partial
        one that follows).  Returns the number of graphs captured.  Failures fall back to eager execution as in `step()`."""
        before = self.captures
        cap = self._capacity()
        if cap is not None and self.capture_error is None and not self._fits(cap):
            self._try_capture(cap)
        if cap is not None and self.graphs is not None and self.capture_error is None and self.capacity_ladder:
            # the ladder: graphs for the capacities the estimate may move to (each rung owns its buffers: ~2 KB per sample and buffer set)
            base = self.captured_capacity
            for f in self.capacity_ladder:
                rung = ((int(base * f) + self.quantum - 1) // self.quantum) * self.quantum
                if rung in self._captured or rung < 16384:
                    continue
                # (what the optimizer recorded about the graphs that stay, should this rung fail half-way: NGPAdam.captures_discarded)
                kept = {k: getattr(self.optimizer, k) for k in ('_poison_captured', '_poisoned') if hasattr(self.optimizer, k)}
                try:
                    self._capture(rung)
                except Exception as e:  # noqa: BLE001 -- the ladder is an optimisation: keep what was captured
                    self.ladder_error = repr(e)
                    for k, v in kept.items():
                        setattr(self.optimizer, k, v)
                    torch.cuda.synchronize()
                    break
            self._activate(base)
        m = self.model
        if self.graphs is not None and self.graph_updates and getattr(m, 'refresh_occupancy', None) is not None and getattr(m, 'cuda_ray', False):
            if update_modes is None:
                update_modes = (True, False) if m.iter_density < 16 else (False,)
            for full in update_modes:
                self._capture_update(bool(full))
        return self.captures - before

    def sync_params(self):
        """make the torch Parameters (and the optimizer's `state`) current after fused-table steps (one host read; optim.NGPAdam.materialize)"""
        fn = getattr(self.optimizer, 'materialize', None)
        if fn is not None:
            fn()

    def _overwrites_table(self):
        """single-GPU direct iteration: the grid backward WRITES the table gradient and the optimizer keeps the buffer (no zeroing, no
        read of the old value: 49 MB per step).  Not with an averager / sharded exchange (they own the flat buffer's life cycle)."""
        import fused
        # (sharded update: the reduce-scatter reads the flat buffer the producers wrote -- every element of it, the MLP regions through the slab
        # reduction -- so the optimizer's memset of that buffer can go as well: NGPAdam.apply(zero=False))
        return bool(fused.USE_OVERWRITE_TABLE and (self.averager is None or self.shards))

    def _mark_deposits(self):
        """after a replay: what the captured optimizer step left in the table's deposit buffer (Python ran only at capture time)"""
        emb = getattr(getattr(self.model, 'encoder', None), 'embeddings', None)
        if emb is not None and self.used_direct and self._overwrites_table():
            from optim import replayed_kept_deposits
            # (sharded update without the memset: every deposit buffer is left as its producer wrote it)
            replayed_kept_deposits([emb] if self.averager is None else [emb] + list(getattr(self.optimizer, 'flat_params', [])))

    def _after_replay(self):
        """what Python would have stated had it issued the step that was just replayed: the deposit buffers the captured optimizer step kept
        (`_mark_deposits`) and, for graphs that carry the table's Adam sweep, that the parity word may have flipped
        (optim.replayed_fused_table_step: `materialize()` reads the word again).  Attribute writes only."""
        self._mark_deposits()
        if self.table_fused:
            from optim import replayed_fused_table_step
            replayed_fused_table_step(self.optimizer)

    def _captures_discarded(self):
        """the graphs are dropped (a failed capture) or about to be recorded anew: the optimizer forgets what it recorded at capture time
        (the command lists go with the record that held the graphs)"""
        fn = getattr(self.optimizer, 'captures_discarded', None)
        if fn is not None:
            fn()

    def _table_fusion_fits(self, emb):
        """does the closing launch of a fused-table step serve THIS table (optim.table_fusion_fits: its dense-level prefix at the captured
        capacity + the other tensors against the cap of ngp_optim_adam_small_commit)?  False as well where the grid backward cannot carry
        the sweep at all: the graphs then keep the separate sweep"""
        import ctypes
        import _ngp_capi as capi
        from fused import network_cfg
        from optim import table_fusion_fits
        m = self.model
        arr = capi.host_offsets(m.encoder.offsets)
        if arr is None:
            return False
        cfg = network_cfg(m.encoder, m.sigma_net, m.color_net, m.bound, True)
        prefix = int(capi.lib.ngp_grid_table_adam_prefix(ctypes.cast(arr, ctypes.c_void_p), int(self.captured_capacity), 3, int(emb.shape[1]), cfg.L,
                                                         cfg.S, cfg.H, cfg.gridtype, cfg.align, capi.NGP_F16))
        rest = sum(p.numel() for p in getattr(self.optimizer, 'flat_params', []) if p is not emb)
        return prefix != 0xffffffff and table_fusion_fits(prefix, emb.shape[1], rest)

    def _cmdlist_ok(self, with_march):
        """THE eligibility of a captured chain for a command list: the autograd-free iteration with producer-checked gradients closed by
        `optimizer.step(gradients_checked=True)`, no GradScaler object, no averager -- what is captured then consists of the library's own
        launches by construction (fused.fused_train_iteration_split, optim.NGPAdam.step): a list records nothing else, so a torch kernel
        in the chain would be lost.  Two places where torch would launch one are excluded: a background-colour TENSOR (converted inside
        the capture) and, where the chain begins with the march (with_march: no lookahead), perturb=False -- the marcher then reads its
        start offsets from a torch.zeros tensor filled inside the capture; with perturb=True it draws them from the seed word.
        Everything else keeps the graph replay: torch.optim, the autograd path, replicated and sharded data-parallel steps.  Call it after
        `_checked_ok` is decided (inside `_capture`)."""
        kw = self.render_kwargs
        if torch.is_tensor(kw.get('bg_color', None)) or (with_march and not kw.get('perturb', False)):
            return False
        return bool(self.use_lists and self.direct and self.scaler is None and self.averager is None and self._checked_ok and self._direct_ok())

    def _recording(self, lists, with_march=False):
        """context of a capture body: records it into a new command list appended to `lists` when the step is eligible, else does nothing"""
        if not self._cmdlist_ok(with_march):
            return contextlib.nullcontext()
        from cmdlist import CommandList
        lists.append(CommandList())
        return lists[-1]

    def _replay_rest(self, g, cl):
        """one step's main chain on the current stream: from its command list where one exists, else the graph"""
        if cl is None:
            g.replay()
        else:
            cl.replay(torch.cuda.current_stream().cuda_stream)
            self.n_list_replays += 1

    def _clean_deposits(self):
        """before replaying graphs whose producers ADD into the deposit buffers: zero what an overwriting producer left behind"""
        clean = getattr(self.optimizer, 'clean_deposits', None)
        if clean is not None and not (self.used_direct and self._overwrites_table()):
            clean(getattr(self.optimizer, 'flat_params', []))

    def _direct_ok(self):
        m, kw = self.model, self.render_kwargs
        if not (self.direct and m.training and getattr(m, 'bg_radius', 0) <= 0 and hasattr(m, '_fused_render_ok')):
            return False
        # geo: the caller wants depth_raw / distortion in the render's results and its own loss on them; the direct iteration serves the
        # geometry terms it knows through `geo_loss` (_iteration_args hands it over: _direct_ok does not depend on it)
        # aux: the caller's own channels are composited on the autograd path only
        if kw.get('staged', False) or kw.get('geo', False) or kw.get('aux', None) is not None:
            return False
        bg = kw.get('bg_color', None)
        with torch.autocast('cuda', dtype=self.autocast_dtype):  # the fused path IS the fp16-autocast arithmetic; it checks for it
            return m._fused_render_ok(self.rays_o.view(-1, 3), self.rays_d.view(-1, 3), 1 if bg is None else bg,
                                      kw.get('force_all_rays', False))

    def _iteration_args(self, checked, p=None):
        """(args, kwargs) of fused.fused_train_iteration / fused_train_iteration_split on the static buffers -- of buffer set `p` of the
        lookahead (its own counter row and noise seed), else of the single set (seeded by the optimizer's step count).
        checked: the producers flag non-finite gradients themselves -- and carry the table's Adam sweep when the graphs were captured for it
        (table_fused; the optimizer is then handed over as `table_adam`, else its separate sweep runs)"""
        from optim import FOUND_INF, SCALE, STEP_COUNT
        m, kw, opt = self.model, self.render_kwargs, self.optimizer
        bg = kw.get('bg_color', None)
        if p is None:
            batch, counter, seed = (self.rays_o, self.rays_d, self.target), self.counter[0], opt.scalars.narrow(0, STEP_COUNT, 1)
        else:
            batch, counter, seed = (self.la_rays_o[p], self.la_rays_d[p], self.la_target[p]), self.counter[p], self.la_seed[p:p + 1]
        args = (m, *batch, m.aabb_train, counter, self.captured_capacity, opt.scalars.narrow(0, SCALE, 1), 1 if bg is None else bg, kw.get('perturb', False),
                kw.get('dt_gamma', 0), kw.get('max_steps', 1024), kw.get('T_thresh', 1e-4))
        return args, dict(noise_seed=seed, found_inf=opt.scalars.narrow(0, FOUND_INF, 1) if checked else None, overwrite_table=self._overwrites_table(),
                          table_adam=opt if checked and self.table_fused else None, geo_loss=self.geo_loss)

    def _iteration_front(self):
        """zero_grad -> render -> loss -> scaled backward, with the model's bookkeeping pinned for capture"""
        m = self.model
        if self._direct_ok():
            from fused import fused_train_iteration
            self.optimizer.zero_grad(set_to_none=True)
            # single rank (or local gradients before a sharded exchange): the producers flag non-finite gradients, no separate sweep.
            # After an all-reduce the sweep has to see the REDUCED values, so the replicated data-parallel path keeps it.
            self.active.producers_check = self._checked_ok and (self.averager is None)
            args, kwargs = self._iteration_args(self.producers_check)
            loss, self.image = fused_train_iteration(*args, **kwargs)[:2]
            self.active.used_direct = True
            return loss[0]
        self._geo_loss_needs_direct()
        self.active.used_direct = False
        self.active.producers_check = False
        saved_counter, saved_mc, saved_ls = m._buffers['step_counter'], m.mean_count, m.local_step
        m._buffers['step_counter'] = self.counter
        m.mean_count = self.captured_capacity - 128  # march_rays_train sizes its buffers as mean_count + 128 (raymarching.py:200-203)
        m.local_step = 0
        try:
            self.optimizer.zero_grad(set_to_none=True)
            with torch.autocast('cuda', dtype=self.autocast_dtype):
                out = m.render(self.rays_o, self.rays_d, **self.render_kwargs)
                loss = self.loss_fn(out, self.target)
            self.image = self._image_of(out)
            self._scaled(loss).backward()
        finally:
            m._buffers['step_counter'], m.mean_count, m.local_step = saved_counter, saved_mc, saved_ls
        return loss

    @staticmethod
    def _image_of(out):
        """the [N,3] image of a render's results as `self.image` holds it: detached, no launch where the renderer returns fp32 (it does)"""
        return out['image'].detach().reshape(-1, 3).float()

    def _geo_loss_needs_direct(self):
        """a geo_loss is served by the autograd-free iteration alone: raise where the graphs about to be captured would leave it out"""
        if self.geo_loss is not None and not self._direct_ok():
            raise RuntimeError('GraphedTrainStep: geo_loss needs the autograd-free iteration and this model / render configuration is not '
                               'eligible for it (GraphedTrainStep._direct_ok)')

    def _scaled(self, loss):
        # torch.optim + GradScaler, or an optimizer that owns its loss scale (optim.NGPAdam: scale / step, no scaler object)
        return self.scaler.scale(loss) if self.scaler is not None else self.optimizer.scale(loss)

    def _iteration_back(self):
        if self.scaler is not None:
            self.scaler.step(self.optimizer)
            self.scaler.update()
        elif self.producers_check:
            self.optimizer.step(gradients_checked=True)
        else:
            self.optimizer.step()

    def _capture(self, cap):
        """capture the training iteration for `cap` samples into a new record, which becomes the active one and joins `_captured`"""
        # No warm-up iterations here: they would be real optimizer steps.  Everything lazily created (optimizer state,
        # GradScaler scale tensor, LDS-size attributes, device properties) exists already because capture only starts once
        # `mean_count > 0`, i.e. after >= 16 eager iterations.  Capturing does not execute: the first replay is the step.
        import gc
        self.captured_capacity = cap
        rec = self.active = _Capture(cap)   # (what the capture bodies read -- _iteration_front, _iteration_args, _cmdlist_ok -- and fill in)
        self.image = None
        gc.collect()  # drop autograd graphs of earlier eager iterations (their AccumulateGrad nodes are stream-bound)
        torch.cuda.synchronize()
        _drain_parked()
        direct = self._direct_ok()
        # (outside capture: caches the host copy of the encoder offsets the in-kernel non-finite sweep needs)
        if direct:
            from fused import iteration_checks_gradients
            rec.checked_ok = iteration_checks_gradients(self.model)
        self.sync_params()   # (outside the capture: a re-capture starts from buffer set A)
        self._captures_discarded()   # (a capture that contains poison_shards() records it again)
        if self.fused_table_adam and rec.checked_ok and self._overwrites_table() and cap >= 16384:
            emb = getattr(getattr(self.model, 'encoder', None), 'embeddings', None)
            if emb is not None and getattr(emb, '_ngp_fp16', None) is not None and self._table_fusion_fits(emb):
                self.optimizer.enable_table_fusion(emb)
                rec.table_fused = True
        self.la_ready = [None, None]
        # THE choice of the replay shape; each shape states its capture and its step side by side below
        if self.lookahead and direct:
            self._capture_lookahead(rec)
        elif self.averager is None:
            self._capture_plain(rec)
        elif self.shards and direct:
            self._capture_sharded(rec)
        else:
            self._capture_replicated(rec)
        self.n_captures += 1
        self._captured[cap] = rec
        while len(self._captured) > 12:   # (an estimate that wanders for a long time: drop the capacity farthest from the active one)
            far = max((c for c in self._captured if c != cap), key=lambda c: abs(c - cap))
            _PARKED.append(self._captured.pop(far))

    def _try_capture(self, cap):
        """capture for `cap` samples -> True; a capture that fails is recorded (`capture_error`: every step from here on runs eagerly), what
        it left is dropped and the optimizer is told.  THE statement of the fallback: `step()` and `precapture()` both come through here"""
        self._geo_loss_needs_direct()
        try:
            self._capture(cap)
            return True
        except Exception as e:  # noqa: BLE001 -- keep training eagerly; the caller can inspect .capture_error
            self.capture_error = repr(e)
            self.active = _Capture()
            self._captures_discarded()
            torch.cuda.synchronize()
            return False

    def _set_batch(self, rays_o, rays_d, target):
        """the batch into the single buffer set: ONE multi-tensor copy kernel (three separate copies cost ~5 us each plus the gaps)"""
        torch._foreach_copy_([self.rays_o, self.rays_d, self.target], [rays_o.view_as(self.rays_o), rays_d.view_as(self.rays_d), target],
                             non_blocking=True)

    def _count_to_ring(self, p=0, ahead=0):
        """hand the sample count of buffer set `p` (0: also the single set) to the model's 16-slot ring exactly where the eager renderer would
        have put it -- ahead=1: the slot the NEXT step will own"""
        m = self.model
        m.step_counter[(m.local_step + ahead) % 16].copy_(self.counter[p], non_blocking=True)

    # ---- plain: one graph (single rank, torch.optim or optim.NGPAdam, with or without the autograd-free iteration) ---------------------
    def _capture_plain(self, rec):
        g = torch.cuda.CUDAGraph()
        lists = []
        with _capture_into(g):
            with self._recording(lists, with_march=True):
                rec.loss = self._iteration_front().detach()
                self._iteration_back()
        rec.graphs, rec.lists, rec.image, rec.replay = (g,), tuple(lists) or None, self.image, GraphedTrainStep._replay_plain

    def _replay_plain(self, rays_o, rays_d, target, next_rays):
        rec = self.active
        (g,), (cl,) = rec.graphs, rec.lists or (None,)
        self.image = rec.image
        self._set_batch(rays_o, rays_d, target)
        self._replay_rest(g, cl)
        self._count_to_ring()
        return rec.loss

    # ---- replicated data-parallel: two graphs, the RCCL all-reduce stays eager between the two halves ------------------------------------
    def _capture_replicated(self, rec):
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with _capture_into(g1):
            rec.loss = self._iteration_front().detach()
        with _capture_into(g2, pool=g1.pool()):
            self._iteration_back()
        rec.graphs, rec.image, rec.replay = (g1, g2), self.image, GraphedTrainStep._replay_replicated

    def _replay_replicated(self, rays_o, rays_d, target, next_rays):
        rec = self.active
        front, back = rec.graphs
        self.image = rec.image
        self._set_batch(rays_o, rays_d, target)
        front.replay()
        self.averager.all_reduce()
        back.replay()
        self._count_to_ring()
        return rec.loss

    # ---- sharded data-parallel update (optim.NGPAdam, shard=True) without lookahead: three graphs around the two collectives -------------
    def _capture_sharded(self, rec):
        #   [march] -> wait for the shadow all-gather of the previous step -> [encode .. backward, local non-finite sweep, poison]
        #   -> reduce-scatter (carries the skip verdict) -> [verdict, Adam on my shard, commit] -> all-gather of the shadows (side stream,
        #   overlaps the next [march]).  This is the form WITHOUT lookahead; with lookahead (the default of bench.py) the march leaves the
        #   main stream altogether: _capture_lookahead.  (Folding the next batch's march behind the shard update -- two replays per step --
        #   was measured over a 1-rank RCCL group and dropped: 0.607 against 0.591 ms, EXPERIMENTS.md round 5.)
        from fused import fused_train_iteration_split
        opt = self.optimizer
        args, kwargs = self._iteration_args(rec.checked_ok)   # (no table fusion here: it needs averager=None)
        march, rest = fused_train_iteration_split(*args, **kwargs)
        opt.wait_shadows()
        torch.cuda.synchronize()
        ga, gb, gc_ = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with _capture_into(ga):
            march()
        with _capture_into(gb, pool=ga.pool()):
            losses, rec.image = rest()[:2]
            rec.loss = losses[0].detach()
            if not rec.checked_ok:
                opt.pre_reduce_check()     # (else the kernels that deposited the local gradients flagged them)
            opt.poison_shards()            # found_inf -> NaN in element 0 of every shard: the reduce-scatter carries the verdict
        with _capture_into(gc_, pool=ga.pool()):
            opt.apply(zero=not self._overwrites_table())
        rec.graphs, rec.sharded, rec.used_direct, rec.replay = (ga, gb, gc_), True, True, GraphedTrainStep._replay_sharded

    def _replay_sharded(self, rays_o, rays_d, target, next_rays):
        # Eager operations between graph replays are where this step loses time (kernel trace of the 1-rank RCCL step,
        # profiles/r05_step_timeline_ddp.txt: a replay that follows an eager kernel starts at once, an eager kernel that follows a replay
        # waits 9-32 us), so the small copies sit BEHIND the eager reduce-scatter, where a boundary exists anyway: the sample count goes
        # to the model's ring there, and an announced next batch (next_rays) is copied into the static buffers there -- the next step then
        # starts with a replay right behind this step's last one.  (rays_o / rays_d are read by the march graph only, the target by the
        # rest graph: both are done with them by then, stream order.)
        rec, opt = self.active, self.optimizer
        march, rest, apply = rec.graphs
        self.image = rec.image
        pc, self._precopied = self._precopied, None
        if not (pc is not None and pc.holds_rays(rays_o, rays_d) and pc.holds_target(target)):
            self._set_batch(rays_o, rays_d, target)
        march.replay()                     # near/far + ray marching: needs no weights, overlaps the shadow all-gather of the last step
        opt.wait_shadows()
        rest.replay()                      # encode .. backward (deposit) + local non-finite sweep + poison
        opt.reduce_gradients()             # reduce-scatter (average of my shard; the skip verdict rides in it)
        self._count_to_ring()
        if next_rays is not None and len(next_rays) > 2:
            self._set_batch(*next_rays)
            self._precopied = _Announced.of(*next_rays)
        apply.replay()                     # verdict + Adam on my shard, scale / step commit, deposit buffer zeroed
        opt.gather_shadows()               # all-gather of the fp16 shadows on the side stream
        return rec.loss

    # ---- lookahead: two buffer sets, per set a march graph and a rest graph; the next batch's march runs on a side stream --------------
    def _capture_lookahead(self, rec):
        """two buffer sets, per set a march graph (static rays of the set -> its samples) and a rest graph (samples + target -> loss,
        gradients, optimizer step).  The march graphs allocate from their own pool: a march replays while the OTHER set's rest graph runs."""
        from fused import fused_train_iteration_split
        opt = self.optimizer
        rec.producers_check = rec.checked_ok
        pool_march, rec.rest_pool = torch.cuda.graph_pool_handle(), torch.cuda.graph_pool_handle()
        # data-parallel sharded update: the rest graph ends with the local non-finite sweep + poison; reduce-scatter -> [apply graph] ->
        # all-gather follow eagerly (or, graph_collectives, inside the rest graph: ONE replay per step on the main stream)
        sharded = self.shards
        if sharded:
            opt.wait_shadows()
            torch.cuda.synchronize()
        la, lists = [], []
        for p in range(2):
            args, kwargs = self._iteration_args(rec.checked_ok, p)   # (a sharded update has no fused table: it needs averager=None)
            march, rest = fused_train_iteration_split(*args, **kwargs)
            gm, gr = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with _capture_into(gm, pool=pool_march):
                march()
            with _capture_into(gr, pool=rec.rest_pool), (contextlib.nullcontext() if sharded else self._recording(lists)):
                opt.zero_grad(set_to_none=True)
                losses, image = rest()[:2]
                if not sharded:
                    self._iteration_back()
                else:
                    if not rec.checked_ok:
                        opt.pre_reduce_check()
                    opt.poison_shards()
                    if self.graph_collectives:
                        opt.reduce_gradients()
                        opt.apply(zero=not self._overwrites_table())
                        opt.gather_shadows(async_op=False)   # same stream: no fork inside the graph
            la.append(_LaSet(gm, gr, losses[0].detach(), image, march, rest))
        if sharded and not self.graph_collectives:
            rec.la_apply = torch.cuda.CUDAGraph()
            with _capture_into(rec.la_apply, pool=rec.rest_pool):
                opt.apply(zero=not self._overwrites_table())
        rec.la, rec.graphs, rec.lists = la, tuple(g for s in la for g in (s.march_graph, s.rest_graph)), tuple(lists) or None
        if rec.lists and MARCH_MARKS[self.march_at] is not None:
            kernel, behind = MARCH_MARKS[self.march_at]
            for cl in rec.lists:   # the event behind (before) the named launch: the side stream's march of the next batch waits for it
                at = [i for i, n in enumerate(cl.names()) if kernel in n]
                if not at:
                    raise RuntimeError(f'GraphedTrainStep: NGP_STEP_MARCH_AT={self.march_at}: no {kernel} launch in the recorded chain')
                cl.mark(MARCH_MARK_ID, max(at) + behind)
        rec.used_direct, rec.replay = True, GraphedTrainStep._replay_lookahead

    def _replay_lookahead(self, rays_o, rays_d, target, next_rays):
        m, rec = self.model, self.active
        p = self.la_cur
        q = 1 - p
        cur = rec.la[p]
        self.image = cur.image   # (this set's static image buffer: written by the rest chain replayed below)
        main = torch.cuda.current_stream()
        ready, self.la_ready[p] = self.la_ready[p], None
        if ready is not None:
            # hit or miss: whatever the side stream was asked to march into set p (its copies into la_rays_*/la_seed[p], the replay of
            # gm_p, the ring-slot hand-over) must have finished before this stream reads OR overwrites that set
            main.wait_event(self.la_event[p])
        if ready is not None and ready.holds_rays(rays_o, rays_d, self.occupancy_epoch):
            if not ready.holds_target(target):      # the target was not announced with the rays: copy it now
                self.la_target[p].copy_(target, non_blocking=True)
            self.la_hits += 1                       # the march of this batch ran on the side stream during the previous step
        else:
            torch._foreach_copy_([self.la_rays_o[p], self.la_rays_d[p], self.la_target[p]],
                                 [rays_o.view_as(self.la_rays_o[p]), rays_d.view_as(self.la_rays_d[p]), target], non_blocking=True)
            self.la_seed[p:p + 1].fill_(self.global_step)
            cur.march_graph.replay()
            self._count_to_ring(p)
            if self.la_slot_event is None:
                self.la_slot_event = torch.cuda.Event()
            self.la_slot_event.record(main)
        ahead = next_rays is not None and (self.global_step + 1) % self.update_interval != 0
        cl = rec.lists[p] if rec.lists else None
        # a marked list: the main chain goes first and the side stream waits for the mark inside it -- later than the step boundary, never
        # earlier (set q was read by the previous step's chain, which `main` holds in front of this one)
        early = ahead and cl is not None and MARCH_MARKS[self.march_at] is not None
        if early:
            self._replay_rest(cur.rest_graph, cl)
        if ahead:
            side = self.la_side
            if early:
                cl.wait_mark(MARCH_MARK_ID, side.cuda_stream)
            else:
                side.wait_stream(main)              # set q was read by the previous step's rest graph, queued on `main` before this point
            with torch.cuda.stream(side):
                no, nd, *nt = next_rays             # the next target too, where it is given: its copy leaves the main stream as well
                dst, src = [self.la_rays_o[q], self.la_rays_d[q]], [no.view_as(self.la_rays_o[q]), nd.view_as(self.la_rays_d[q])]
                torch._foreach_copy_(dst + [self.la_target[q]] * len(nt), src + nt, non_blocking=True)
                self.la_seed[q:q + 1].fill_(self.global_step + 1)
                rec.la[q].march_graph.replay()
                self._count_to_ring(q, ahead=1)     # the sample count of the next step goes to the model's ring from here
                self.la_event[q].record(side)
            self.la_ready[q] = _Announced.of(no, nd, *nt, epoch=self.occupancy_epoch)
        elif (self.global_step + 1) % self.update_interval == 0 and self.graph_updates and self.update_capture_error is None:
            # the next step starts with an occupancy refresh: its weight-independent half (which cells, where inside them) runs here instead
            full = m.iter_density < 16
            entry = self.update_graphs.get(full)
            if entry is not None and entry.sampling is not None:
                side = self.la_side
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    entry.sampling.replay()
                    self.la_sample_event.record(side)
                self.la_presampled = full
        if rec.la_apply is not None:           # sharded update, eager collectives: [rest] -> reduce-scatter -> [apply] -> all-gather (side stream)
            opt = self.optimizer
            opt.wait_shadows()
            cur.rest_graph.replay()
            opt.reduce_gradients()
            rec.la_apply.replay()       # (issued eagerly instead -- one replay boundary less, three eager launches more: 0.530 against 0.516 ms, EXPERIMENTS.md)
            opt.gather_shadows()
        elif not early:
            self._replay_rest(cur.rest_graph, cl)
        self.la_cur = q
        return cur.loss

    def _capture_update(self, full):
        """record the occupancy refresh into graphs of its own (nothing executes); False when capture is not possible.  Lookahead mode
        records its two halves separately -- (cell sampling, pool of its own: replays on the side stream under a training iteration) and
        (density evaluation + grid / bitfield update) -- otherwise one graph."""
        if full in self.update_graphs:
            return True
        if self.update_capture_error is not None or self.graphs is None:
            return False
        try:
            import gc
            gc.collect()
            torch.cuda.synchronize()
            m = self.model
            if getattr(m, 'fused_refresh', True) and getattr(m, 'density_grid', None) is not None and m.density_grid.is_cuda:
                import raymarching   # the refresh's persistent scratch exists before anything is captured
                raymarching.density_grid_state(m.density_grid, m.__dict__.setdefault('_refresh_state', {}))
            if self.la is not None and hasattr(m, 'refresh_sample'):
                gs, ga = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                if self._sample_pool is None:
                    self._sample_pool = torch.cuda.graph_pool_handle()
                with _capture_into(gs, pool=self._sample_pool):
                    samples = m.refresh_sample(full=full)
                with _capture_into(ga, pool=self.active.rest_pool):
                    with torch.autocast('cuda', dtype=self.autocast_dtype):
                        mean = m.refresh_apply(samples)
                self.update_graphs[full] = _Refresh(ga, mean, gs, samples)
            else:
                g = torch.cuda.CUDAGraph()
                first, *_ = self.graphs   # (the refresh joins the pool of the active capture's first graph)
                with _capture_into(g, pool=first.pool()):
                    with torch.autocast('cuda', dtype=self.autocast_dtype):
                        mean = m.refresh_occupancy(full=full)
                self.update_graphs[full] = _Refresh(g, mean)
            self.n_update_captures += 1
            return True
        except Exception as e:  # noqa: BLE001 -- keep refreshing eagerly; the caller can inspect .update_capture_error
            self.update_capture_error = repr(e)
            torch.cuda.synchronize()
            return False

    def _update_extra_state(self):
        """the occupancy refresh at the Trainer's cadence.  Its device part (model.refresh_occupancy: ~50 small launches around one
        big density evaluation, no host synchronisation) is replayed from a HIP graph of its own once training runs from graphs -- issued
        eagerly it leaves the GPU idle for about half of its 1.2 ms; the host part (sample-count estimate) stays eager."""
        m = self.model
        refresh = getattr(m, 'refresh_occupancy', None)
        if refresh is None or not getattr(m, 'cuda_ray', False):
            with torch.autocast('cuda', dtype=self.autocast_dtype):
                m.update_extra_state()
            return
        full = m.iter_density < 16
        use_graph = self.graph_updates and self.graphs is not None and self.update_capture_error is None
        if use_graph and full not in self.update_graphs:
            use_graph = self._capture_update(full)
        mean_count = None
        if use_graph and self.la is not None and m.local_step > 0:
            # the sample-count estimate is a host read-back (renderer.py:531-538).  Read through the main stream it waits for everything
            # queued there -- the steps the host is ahead by and the refresh itself -- and the GPU then idles until the host has issued the
            # next step.  The counts were written by the march launches, on the side stream (or, for a step whose batch was not announced,
            # early on the main stream: la_slot_event): reading them on the side stream waits for those only, the main stream keeps its
            # backlog.  Same numbers, read before the refresh is queued instead of after.
            used = min(16, m.local_step)
            with torch.cuda.stream(self.la_side):
                if self.la_slot_event is not None:
                    self.la_side.wait_event(self.la_slot_event)
                mean_count = int(m.step_counter[:used, 0].sum().item() / used)
        if use_graph:
            entry = self.update_graphs[full]
            mean = entry.mean
            if entry.sampling is not None:           # split refresh: the sampling half may already have run under the previous iteration
                if self.la_presampled == full:
                    torch.cuda.current_stream().wait_event(self.la_sample_event)
                    self.la_presample_hits += 1
                else:
                    entry.sampling.replay()
                self.la_presampled = None
            entry.graph.replay()
        else:
            with torch.autocast('cuda', dtype=self.autocast_dtype):
                mean = refresh(full=full)
        m.finish_update(mean, mean_count=mean_count)   # (None: the model reads the ring itself)

    def _eager(self, rays_o, rays_d, target):
        self.optimizer.zero_grad(set_to_none=True)
        geo = self.geo_loss
        with torch.autocast('cuda', dtype=self.autocast_dtype):
            if geo is None:
                out = self.model.render(rays_o, rays_d, **self.render_kwargs)
                loss = self.loss_fn(out, target)
            else:   # the same term through autograd (the steps before the sample estimate exists)
                out = self.model.render(rays_o, rays_d, **dict(self.render_kwargs, geo=True))
                loss = self.loss_fn(out, target) + geo.lambda_distortion * out['distortion'].float().mean()
        self.image = self._image_of(out)
        self._scaled(loss).backward()
        if self.averager is not None and not getattr(self.optimizer, 'shard', False):
            self.averager.all_reduce()
        self._iteration_back()  # (a sharded optim.NGPAdam exchanges inside step(): reduce-scatter, update, all-gather)
        # detached: a caller holding the loss must not keep this iteration's autograd graph (and its AccumulateGrad nodes,
        # bound to the eager stream) alive into a later capture
        return loss.detach()

    # ------------------------------------------------------------------------------------------
    def _ready_for(self, cap):
        """make a capture that serves an estimate of `cap` samples the active one: the active one where it still fits, else another captured
        capacity (a switch: no capture, no device work), else a new capture.  False: nothing is captured, the step runs eagerly"""
        if self._fits(cap):
            return True
        pick = self._pick_captured(cap)
        if pick is None:
            return self._try_capture(cap)
        if pick != self.captured_capacity:
            self._activate(pick)
        return True

    def step(self, rays_o, rays_d, target, next_rays=None):
        """one training iteration on rays_o/rays_d [1,N,3], target [N,3]; returns the (device) loss of this step.  Afterwards `self.image` is
        the step's finished [N,3] fp32 image (a view of a static buffer: valid until the next step()).
        next_rays=(rays_o, rays_d[, target]) of the FOLLOWING step (lookahead=True only): marched (and, with the target, staged) on a side
        stream under this iteration; the following step recognises the batch by the identity of these tensors."""
        m = self.model
        if self.global_step % self.update_interval == 0:
            if getattr(self.optimizer, 'shard', False):
                self.optimizer.wait_shadows()  # the occupancy refresh evaluates the density network on the fp16 shadows
            if self.la is not None:
                torch.cuda.current_stream().wait_stream(self.la_side)
            self._update_extra_state()
            self.occupancy_epoch += 1
            if self.after_update is not None:
                self.after_update(m)
        self.capacity = cap = self._capacity()
        # eager: no sample estimate yet, or a capture failed (now or earlier: stay on the eager path)
        if cap is None or self.capture_error is not None or not self._ready_for(cap):
            loss = self._eager(rays_o, rays_d, target)
        else:
            self.capacity = self.captured_capacity
            self._clean_deposits()
            loss = self.active.replay(self, rays_o, rays_d, target, next_rays)
            self._after_replay()
            m.local_step += 1    # (the eager render counts its own steps)
        self.global_step += 1
        return loss
