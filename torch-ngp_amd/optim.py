"""Fused Adam + dynamic loss scaling for the instant-ngp parameter set over `ngp_optim_adam_step`.

Replaces the pair the reference trains with -- `torch.optim.Adam(..., betas=(0.9, 0.99), eps=1e-15)` (main_nerf.py:132) and
`torch.cuda.amp.GradScaler` (nerf/utils.py:393, 557-560) -- by ONE object with the three calls a training loop needs:

    opt = NGPAdam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
    opt.zero_grad();  opt.scale(loss).backward();  opt.step()          # = scaler.scale / scaler.step / scaler.update

Same update rule as PyTorch's Adam and the same scale dynamics as GradScaler (x2 after 2000 clean steps, x0.5 and a skipped step
when any gradient is non-finite); everything stays on the device (no `.item()`), so the step can be captured in a HIP graph.

What it removes on the 12.24 M-entry hash table, per iteration: the fp16 gradient memset, autograd's fp16->fp32 gradient cast, the
separate non-finite sweep over an fp32 gradient, the unscaled-gradient write-back of the fused Adam kernel, and the fp32->fp16
cast of the table before the next forward.  Mechanism: every parameter gets an fp16 shadow copy (`p._ngp_fp16`, refreshed by the
update kernel) and an fp16 gradient buffer (`p._ngp_grad16`, zeroed by the update kernel).  The fused Functions in fused.py read
the shadow instead of casting and let the backward kernels write straight into the gradient buffer (returning no autograd
gradient for that parameter).  Parameters whose gradient arrives the ordinary way (`p.grad`, fp32 -- the module-by-module path)
are handled by the same kernel.  With gradient deposit, run ONE backward per step (the MLP weight gradients are accumulated by the
kernels, but a second backward before `step()` would also re-read stale shadows).

Multi-GPU (one process per GPU, torch.distributed; 'nccl' is RCCL over xGMI), two modes:
  * replicated (`shard=False`): `all_reduce()` AVERAGES the one flat fp16 gradient buffer over ranks (24.5 MB instead of 49 MB of fp32):
    RCCL's AVG pre-multiplies by 1/world before summing, so the loss-scaled fp16 sum cannot overflow where a single rank's gradient did
    not (a plain SUM of 8 x 65536-scaled gradients would); every rank then runs the full update.
  * sharded (`shard=True`, ZeRO-1 style): the flat buffer is cut into world_size equal shards; `reduce_gradients()` = ONE
    reduce-scatter (each rank receives the average of its shard), the rank updates only its 1/world of the moments, fp32 master weights
    and fp16 shadows (Adam's 30 B/parameter sweep shrinks by world_size), and `gather_shadows()` = ONE all-gather of the fp16 shadows
    on a side stream, which the next iteration's parameter-independent ray marching overlaps.  Same bytes on the wire as the ring
    all-reduce (which is a reduce-scatter + all-gather), 1/world of the optimizer traffic, and the gather leaves the critical path.
    The "step skipped as a whole" rule needs a global verdict: every rank sweeps its LOCAL gradient before the exchange into found_inf
    (the FOUND_INF word of `scalars`); `poison_shards()` then writes NaN into the first element of every shard when that flag is set, the reduce-scatter carries
    the NaN to every owner, and `apply()` reads the global verdict off its own shard (`verdict='poison'`, the default: no collective besides
    the reduce-scatter on the critical path).  `verdict='allreduce'` keeps round 3's extra 4-byte all_reduce(MAX) next to the reduce-scatter.
    `shard='force'` runs this path on ONE rank as well (a 1-rank process group: every collective executes, the exchange is the identity) --
    bench.py's `ddp_overhead_1rank` and tests/test_gpu_ddp.py, the only way to execute RCCL on a one-GPU box.
    The fp32 parameters are re-pointed into one flat master buffer (`gather_master()` completes them on every rank for checkpoints).

The deposit hand-off: who may write which mark when.  The gradient producers (fused.py; graph.py after a replay) and this optimizer agree
on the state of a parameter's fp16 gradient buffer `p._ngp_grad16` through marks on the torch Parameter.  Producers set them only through
the functions below (tests and tools that play producer assign them directly):

| state of the buffer | marks on the Parameter | entered by |
|---|---|---|
| clean (all zero) | neither | the update kernel's zeroing (`step()`, `apply(zero=True)`); `clean_deposits()` on a stale buffer |
| added-into | neither | an adding producer (the autograd Functions of fused.py), which asks for `clean_deposits()` first |
| overwritten this step | `_ngp_deposit_overwritten` | `announce_overwrite()`: the producer wrote every element and read none (`overwrite_table`) |
| stale (a consumed gradient) | `_ngp_grad16_stale` | `step()` / `apply(zero=False)` on an overwritten buffer: kept, not zeroed; `replayed_kept_deposits()` after a graph replay of the two |

A stale buffer goes back to overwritten (the next overwriting producer) or to clean (`clean_deposits()`: asked for by an adding producer,
and by `step()` itself for every buffer nobody announced).  A consumer that meets a stale buffer nobody refreshed refuses
(`_refuse_stale_deposits`: it would apply the previous step's gradient a second time, or average it).  `announce_overwrite(p, prefix)`
also carries the table sweep: `_ngp_table_adam_done` (the producer's grid backward applied Adam to the table, the next `step()` is the small
closing launch and resets the mark) and `_ngp_table_adam_prefix` (the dense-level entries at the start of the table, which that launch
sweeps).  The shadow half of the contract: `p._ngp_fp16` is current while `p._ngp_version == p._version` (`refresh_shadow`,
`resync_stale_shadows`).  One host flag belongs to the same hand-off: `NGPAdam._maybe_flipped`, set by `table_adam()` ("a fused-table step
was issued": buffer set B may be the current one) and cleared by `materialize()`.  Python runs `table_adam()` at capture time only, so
whoever REPLAYS a captured fused-table step states it after every replay (`replayed_fused_table_step()`): `materialize()` then reads the
parity word again (tests/test_gpu_table_adam.py: every reader and writer outside the graphs at odd and even replay counts).
"""
import collections
import ctypes

import torch
import torch.distributed as dist

import _ngp_capi as capi

_MAX = 8

# the eight device-resident state words of an optimizer (`NGPAdam.scalars`; layout and meaning: include/ngp_hip.h, ngp_optim_adam_step);
# `scalars.narrow(0, WORD, 1)` is the one-element view that kernels and in-place writes take
SCALE, GROWTH_TRACKER, FOUND_INF, STEP_COUNT, LR_MULT, TABLE_PARITY, TICKET, SCALE_DEAD = range(8)


# one tensor of a launch: flat tensors (param / moments / shadows may be None), grad_is_half bits (1: fp16 gradient, 2: kept, not zeroed)
Entry = collections.namedtuple('Entry', 'n param exp_avg exp_avg_sq grad fp16 is_half lr ema')


def _entry_arrays(entries, ema, keep):
    """up to 8 `Entry`s as nine void* in the order of the fields (ctypes arrays, appended to `keep`: alive until the caller drops them); the
    EMA shadows only with `ema` (else None); all None for a launch without entries"""
    k, vp = len(entries), ctypes.c_void_p
    if not k:
        return [None] * 9
    ptrs = lambda tensors: (vp * k)(*[(t.data_ptr() if t is not None else None) for t in tensors])
    col = Entry(*zip(*entries))   # one tuple per field
    arrs = ((ctypes.c_uint64 * k)(*map(int, col.n)), ptrs(col.param), ptrs(col.exp_avg), ptrs(col.exp_avg_sq), ptrs(col.grad), ptrs(col.fp16),
            (ctypes.c_int * k)(*map(int, col.is_half)), (ctypes.c_float * k)(*map(float, col.lr)), ptrs(col.ema) if ema else None)
    keep.append((arrs, entries))
    return [ctypes.cast(a, vp) if a is not None else None for a in arrs]


def announce_overwrite(p, table_adam_prefix=None):
    """a producer WROTE the whole deposit buffer of `p` this step: the next step()/apply keeps the buffer instead of zeroing it.
    table_adam_prefix: the producer's grid backward also applied Adam to the table `p`, except its first `table_adam_prefix` entries (the
    dense levels: ngp_grid_table_adam_prefix) -- the next step() sweeps those in its closing launch and leaves the rest alone"""
    p._ngp_deposit_overwritten = True
    if table_adam_prefix is not None:
        p._ngp_table_adam_prefix = int(table_adam_prefix)
        p._ngp_table_adam_done = True


def _consumed(p, kept):
    """step() / apply() handed the deposit buffer of `p` to the update kernel, which zeroed it (clean) or kept it (stale from here on)"""
    p._ngp_deposit_overwritten = False
    p._ngp_grad16_stale = kept


def replayed_kept_deposits(params):
    """after the replay of a captured step() / apply(zero=False) behind overwriting producers: Python ran at capture time only, so the
    overwritten -> stale transition of every replay is stated here"""
    for p in params:
        if getattr(p, '_ngp_grad16', None) is not None:
            p._ngp_grad16_stale = True


def replayed_fused_table_step(optimizer):
    """after the replay of a captured fused-table iteration (`table_adam()` handed to the grid backward + the closing launch): the device
    may have flipped the parity word, buffer set B may be the current one -- what `table_adam()` recorded when Python issued the step.
    One attribute write, no device work; `materialize()` reads the word the next time somebody outside the graphs asks for the table"""
    if getattr(optimizer, 'fused_table', None) is not None:
        optimizer._maybe_flipped = True


# ngp_optim_adam_small_commit (csrc/optim.hip: NGP_REQUIRE(total <= (1u << 22))) serves the closing launch of a fused-table step up to this
# many parameters: the table's dense-level prefix plus the remaining tensors
SMALL_COMMIT_MAX_PARAMS = 1 << 22


def table_fusion_fits(prefix_entries, level_dim, rest_params):
    """can the closing launch of a fused-table step carry what the grid backward leaves to it?  prefix_entries: the dense-level entries
    at the start of the table (ngp_grid_table_adam_prefix), level_dim: features per entry, rest_params: elements of the optimizer's
    other tensors.  Asked BEFORE `enable_table_fusion` (graph.GraphedTrainStep._capture): a table that does not fit keeps the separate
    sweep instead of failing in step()"""
    return int(prefix_entries) * int(level_dim) + int(rest_params) <= SMALL_COMMIT_MAX_PARAMS


def clean_deposits(params):
    """zero the fp16 deposit buffers that an overwriting producer left stale, before a producer that ADDS into them or a step without a
    fresh deposit; a no-op otherwise (one Python attribute check per parameter)"""
    for p in params:
        if getattr(p, '_ngp_grad16_stale', False):
            p._ngp_grad16.zero_()
            p._ngp_grad16_stale = False


def refresh_shadow(p):
    """the fp16 shadow of `p` from its fp32 value, and the version it was taken at"""
    p._ngp_fp16.copy_(p.detach())
    p._ngp_version = p._version


def resync_stale_shadows(params):
    """NGPAdam updates parameters and fp16 shadows together through raw pointers (no autograd version bump); any OTHER in-place write
    to a parameter (load_state_dict, manual init) bumps `p._version` -- refresh the shadow then, instead of silently using stale weights"""
    for p in params:
        if getattr(p, '_ngp_fp16', None) is not None and getattr(p, '_ngp_version', None) != p._version:
            with torch.no_grad():
                refresh_shadow(p)


class NGPAdam:
    _require_cuda = True   # tests of the multi-rank orchestration subclass this with a torch stand-in for the kernels (tests/ only)

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, world_size=1, deposit=True, shard=False, rank=None, process_group=None, verdict='poison'):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{'params': groups}]
        self.param_groups = []
        for g in groups:
            ps = [p for p in g['params'] if p.requires_grad]
            self.param_groups.append({'params': ps, 'lr': float(g.get('lr', lr))})
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), float(growth_interval)
        self.world_size = int(world_size)
        self.group = process_group
        self.shard = bool(shard) and (self.world_size > 1 or shard == 'force')
        if verdict not in ('poison', 'allreduce'):
            raise ValueError("NGPAdam: verdict must be 'poison' or 'allreduce'")
        self.verdict = verdict
        if self.shard and not deposit:
            raise RuntimeError('NGPAdam: shard=True needs deposit=True (the flat fp16 gradient buffer is what gets reduce-scattered)')
        self.rank = (dist.get_rank(process_group) if rank is None else int(rank)) if self.shard else 0
        self.check_mixed_gradients = False  # debugging aid: costs a device read-back per deposited parameter and step
        self.state = {}
        dev = None
        flat_params = [p for g in self.param_groups for p in g['params']]
        for p in flat_params:
            if not ((p.is_cuda or not self._require_cuda) and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError('NGPAdam: parameters must be contiguous float32 CUDA tensors')
            dev = p.device
        self.flat_params = flat_params
        # packed coordinates: parameter k occupies [offsets[k], offsets[k] + numel) of every flat buffer (slices 16-byte aligned)
        self.offsets, total = [], 0
        for p in flat_params:
            self.offsets.append(total)
            total += (p.numel() + 7) // 8 * 8
        self.payload = total
        if self.shard:  # world_size equal shards of the packed range (a parameter may straddle a boundary)
            self.payload = ((total + self.world_size - 1) // self.world_size + 7) // 8 * 8
            total = self.payload * self.world_size
        self.total = total
        # ONE contiguous fp16 gradient buffer and ONE fp16 shadow buffer: one collective message each per step
        self.flat_grad16 = self.flat_p16 = self.flat_master = None
        if deposit:
            self.flat_grad16 = torch.zeros(total, dtype=torch.half, device=dev)
            self.flat_p16 = torch.zeros(total, dtype=torch.half, device=dev)
        if self.shard:
            self.flat_master = torch.zeros(total, dtype=torch.float32, device=dev)
            self.shard_grad = torch.zeros(self.payload, dtype=torch.half, device=dev)     # my averaged shard (reduce-scatter output)
            self.exp_avg = torch.zeros(self.payload, dtype=torch.float32, device=dev)     # moments of my shard only
            self.exp_avg_sq = torch.zeros(self.payload, dtype=torch.float32, device=dev)
            self.shard_range = (self.rank * self.payload, (self.rank + 1) * self.payload)
        for p, off in zip(flat_params, self.offsets):
            n = p.numel()
            st = {}
            if self.shard:
                self.flat_master[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.flat_master[off:off + n].view_as(p)  # the parameter now lives in the flat master buffer
            else:
                st.update(exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
            if deposit:
                st['fp16'] = self.flat_p16[off:off + n].view_as(p)
                st['fp16'].copy_(p.detach())
                st['grad16'] = self.flat_grad16[off:off + n].view_as(p)
                p._ngp_fp16, p._ngp_grad16, p._ngp_version = st['fp16'], st['grad16'], p._version
            self.state[p] = st
        # the device-resident state words (SCALE ... SCALE_DEAD above; schedulers write LR_MULT)
        self.scalars = torch.tensor([{SCALE: init_scale, LR_MULT: 1.0}.get(i, 0.0) for i in range(8)], dtype=torch.float32, device=dev)
        self._scale_view = self.scalars[SCALE]
        self._keep = []   # ctypes argument arrays of the launches of the current step (kept alive until the next step / building block)
        self._comm_stream = None
        self._shadows_ready = None
        self.fused_table = None       # the parameter whose Adam sweep rides in the grid backward (enable_table_fusion)
        self._table_alt = None        # its second buffer set {'p', 'm', 'v', 'p16'}
        self._maybe_flipped = False   # a fused step was issued since the last materialize(): buffer set B may be the current one

    # -- the table's Adam sweep inside the grid backward (speculative double buffer; include/ngp_hip.h: ngp_table_adam_t) ----------
    def enable_table_fusion(self, param):
        """`param` (the hash table: a deposit-managed parameter of this optimizer) gets a SECOND set of master weights, moments and fp16
        shadow.  A training iteration that passes `table_adam()` to the grid backward (fused.fused_train_iteration(table_adam=...)) has the
        slice accumulate apply Adam to the table in its flush -- reading the set the device-side parity word (TABLE_PARITY) names, writing the
        other -- and `step()` then runs one small launch (Adam on the remaining tensors, loss-scale commit, parity flip when the step
        stands).  GradScaler's skip-the-whole-step rule holds exactly: a skipped step never flips, the current set is never written.
        Outside a stretch of fused steps set A (the torch Parameter, `state[p]`) is the current one: `materialize()` restores that.
        Single-process, non-sharded optimizers only.  Idempotent; +14 B per table parameter of device memory."""
        if self.shard or self.world_size > 1:
            raise RuntimeError('NGPAdam.enable_table_fusion: the sharded / data-parallel update exchanges the gradient first (not available)')
        st = self.state.get(param)
        if st is None or 'fp16' not in st or 'exp_avg' not in st:
            raise RuntimeError('NGPAdam.enable_table_fusion: the parameter is not a deposit-managed parameter of this optimizer')
        if self.fused_table is param:
            return
        if self.fused_table is not None:
            raise RuntimeError('NGPAdam.enable_table_fusion: one table per optimizer')
        self._table_alt = {'p': torch.empty_like(param.data), 'm': torch.empty_like(st['exp_avg']), 'v': torch.empty_like(st['exp_avg_sq']),
                           'p16': torch.empty_like(st['fp16'])}
        for t in self._table_alt.values():
            t.zero_()
        self.fused_table = param
        self.scalars.narrow(0, TABLE_PARITY, 1).zero_()
        # readers of the fp16 table (fused.py: ngp_grid_encode_forward_sel) find the second copy and the parity word on the shadow tensor itself
        st['fp16']._ngp_sel = (self._table_alt['p16'], self.scalars.narrow(0, TABLE_PARITY, 1))
        param._ngp_materialize = self.materialize

    def table_adam(self):
        """ctypes ngp_table_adam_t for the grid backward of this step's iteration (None when no table is fused); marks the step as fused"""
        if self.fused_table is None:
            return None
        self._maybe_flipped = True
        return self._table_adam_struct()

    def _table_adam_struct(self):
        """the struct alone, nothing marked (the closing launch of a fused step takes it too, for the table's dense-level prefix)"""
        p = self.fused_table
        st, alt = self.state[p], self._table_alt
        lr = [g['lr'] for g in self.param_groups if any(q is p for q in g['params'])][0]
        ta = capi.TableAdam()
        ta.param[0], ta.param[1] = p.data.data_ptr(), alt['p'].data_ptr()
        ta.exp_avg[0], ta.exp_avg[1] = st['exp_avg'].data_ptr(), alt['m'].data_ptr()
        ta.exp_avg_sq[0], ta.exp_avg_sq[1] = st['exp_avg_sq'].data_ptr(), alt['v'].data_ptr()
        ta.param_fp16[0], ta.param_fp16[1] = st['fp16'].data_ptr(), alt['p16'].data_ptr()
        ta.state = self.scalars.data_ptr()
        ta.lr, ta.beta1, ta.beta2, ta.eps = float(lr), self.betas[0], self.betas[1], self.eps
        return ta

    @torch.no_grad()
    def materialize(self):
        """after a stretch of fused-table steps: make buffer set A (the torch Parameter, its moments in `state`, its fp16 shadow) the
        current one again -- one host read of the parity word and, when it says B, four device copies.  Called by everything that
        reads or writes the parameter outside the fused iteration (unfused step(), state_dict(), shadow syncs, checkpoints, the fp16 pin
        of an inference render).  Not capturable (it reads the device); a no-op when no fused step ran since the last call."""
        if not self._maybe_flipped or self.fused_table is None:
            return
        if self.scalars.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('NGPAdam.materialize: called inside a stream capture (it reads the parity word on the host)')
        p = self.fused_table
        st, alt = self.state[p], self._table_alt
        if float(self.scalars[TABLE_PARITY].item()) != 0.0:
            p.data.copy_(alt['p'])        # (.data: no autograd version bump -- the shadow is copied right here)
            st['exp_avg'].copy_(alt['m'])
            st['exp_avg_sq'].copy_(alt['v'])
            st['fp16'].copy_(alt['p16'])
            self.scalars.narrow(0, TABLE_PARITY, 1).zero_()
        self._maybe_flipped = False

    # -- GradScaler-like surface -------------------------------------------------------------------
    def scale(self, loss):
        return loss * self._scale_view

    def get_scale(self):
        return float(self.scalars[SCALE].item())

    def scale_is_dead(self):
        """True once the loss scale has underflowed (a long run of overflowing steps halved it to 0 / a denormal): from then on every step is
        skipped -- as with GradScaler, which has no lower bound either -- and nothing else would say so (one host read of the SCALE_DEAD word)"""
        return bool(self.scalars[SCALE_DEAD].item() != 0.0)

    def set_lr_scale(self, factor):
        """multiplies every group's lr (what the reference's LambdaLR does, main_nerf.py:137); a device write, valid under graph replay"""
        self.scalars.narrow(0, LR_MULT, 1).fill_(float(factor))

    def set_lr_lambda(self, fn):
        """`fn(step) -> factor`: the reference's LambdaLR rule (main_nerf.py:137: 0.1 ** min(step / iters, 1)); `schedule_step(step)`
        evaluates it on the host and writes the device multiplier (valid under graph replay)"""
        self._lr_lambda = fn

    def schedule_step(self, step):
        fn = getattr(self, '_lr_lambda', None)
        if fn is not None:
            self.set_lr_scale(fn(int(step)))

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.zero_()
        # the fp16 deposit buffers were zeroed by the last update kernel

    def sync_shadows(self):
        """refresh the fp16 shadow copies after the fp32 parameters were changed from outside (checkpoint load, manual init).
        Sharded mode: a rank keeps only its own 1/world of the fp32 master weights current between steps, so the regions it does not own
        are first completed from their owners (`gather_master()`, a collective: call on every rank) -- otherwise stale master values
        would overwrite the freshly all-gathered shadows.  `assume_complete=True` skips that when the caller has just written the whole
        parameter set itself on every rank (checkpoint load)."""
        self._sync_shadows()

    def _sync_shadows(self, assume_complete=False):
        self.materialize()
        self.wait_shadows()
        if self.shard and not assume_complete:
            self.gather_master()
        for p, st in self.state.items():
            if 'fp16' in st:
                refresh_shadow(p)

    # -- gradient exchange ---------------------------------------------------------------------------
    def _avg_native(self):
        return dist.get_backend(self.group) == 'nccl'  # RCCL: AVG = pre-multiply by 1/world, then sum (no fp16 overflow of the sum)

    @torch.no_grad()
    def all_reduce(self):
        """replicated mode: average the gradients over ranks (call between backward and step).  The loss-scaled fp16 buffer is
        pre-multiplied by 1/world (inside RCCL's AVG, or explicitly on backends without it) BEFORE the sum: exact for power-of-two
        world sizes, and the sum cannot overflow fp16 where no single rank's gradient did."""
        if self.world_size <= 1:
            return
        if self.shard:
            raise RuntimeError('NGPAdam: sharded mode exchanges gradients with reduce_gradients() / step()')
        eager = [p for g in self.param_groups for p in g['params'] if p.grad is not None]
        self._refuse_stale_deposits('all_reduce')
        for p in eager:
            self._average(p.grad)
        if self.flat_grad16 is not None and len(eager) < len(self.state):
            self._average(self.flat_grad16)

    def _refuse_stale_deposits(self, what):
        """the overwrite-table protocol (fused.USE_OVERWRITE_TABLE) leaves a deposit buffer STALE after the step that kept it; every producer
        of the repository either overwrites it again (and says so: announce_overwrite) or zeroes it first.  A consumer that meets a
        stale buffer nobody has refreshed would average / apply the PREVIOUS step's gradient: refuse loudly"""
        for p in self.flat_params:
            if getattr(p, '_ngp_grad16_stale', False) and not getattr(p, '_ngp_deposit_overwritten', False):
                raise RuntimeError(f'NGPAdam.{what}: the fp16 gradient buffer of a parameter is stale (an overwriting producer ran in an earlier '
                                   'step and nothing has written or cleaned it since) -- call clean_deposits() before a producer that adds')

    def _average(self, t):
        if self._avg_native():
            dist.all_reduce(t, op=dist.ReduceOp.AVG, group=self.group)
        else:
            t.mul_(1.0 / self.world_size)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)

    # ---- sharded mode: pre_reduce_check (capturable) -> reduce_gradients (collectives) -> apply (capturable) -> gather_shadows (async) ----
    @torch.no_grad()
    def pre_reduce_check(self):
        """sweep the LOCAL flat gradient for non-finite values into the FOUND_INF word; capturable.  First building block of a
        sharded step: starts a fresh list of kept-alive launch arguments."""
        self._keep = []
        self._launch([Entry(self.total, None, None, None, self.flat_grad16, None, 1, 0.0, None)], capi.NGP_OPT_PHASE_CHECK, 0.0)

    @torch.no_grad()
    def poison_shards(self):
        """verdict='poison': found_inf of the LOCAL gradient (set by the producers or by pre_reduce_check) -> NaN in element 0 of every shard
        of the flat gradient, so that the reduce-scatter hands the verdict to every rank; capturable (one tiny launch), a no-op otherwise"""
        if self.verdict == 'poison':
            self._poison_launch()
            if self.flat_grad16.is_cuda and torch.cuda.is_current_stream_capturing():
                self._poison_captured = True   # part of a graph: every replay issues it
            self._poisoned = True   # (host-side: reduce_gradients() refuses to run without it -- at capture time for a captured step)

    def captures_discarded(self):
        """the graphs that replayed this optimizer's building blocks were dropped or are about to be captured anew (graph.GraphedTrainStep:
        `_capture()`, a failed capture): what capture time recorded about them no longer holds.  A poison launch that was part of a graph
        is not issued any more, so `reduce_gradients()` asks for `poison_shards()` again (a new capture that contains it says so itself)"""
        self._poison_captured = False
        self._poisoned = False

    def _poison_launch(self):
        capi.check(capi.lib.ngp_optim_poison_shards(self.flat_grad16.data_ptr(), self.world_size, self.payload, self.scalars.data_ptr(), capi.stream()))

    def _verdict_launch(self):
        capi.check(capi.lib.ngp_optim_shard_verdict(self.shard_grad.data_ptr(), self.scalars.data_ptr(), self.flat_grad16.data_ptr(), self.world_size,
                                                    self.payload, capi.stream()))

    @torch.no_grad()
    def reduce_gradients(self):
        """ONE reduce-scatter: every rank receives the average of its shard of the flat fp16 gradient.  verdict='allreduce': the per-rank
        found_inf verdicts are combined (MAX) by a second, 4-byte collective so that a step is skipped on all ranks or on none;
        verdict='poison': the reduce-scatter itself carried the verdict (poison_shards before it, apply() reads it)"""
        if self.verdict == 'poison' and not getattr(self, '_poisoned', False):
            # without poison_shards() in front of it the exchange carries NO skip verdict -- the rank that saw the overflow would
            # skip and back off alone, the others would update: parameters and loss scales diverge silently.  (A captured rest graph that ends
            # in poison_shards() sets the flag once, at capture time, and keeps it: the launch is part of every replay.)
            raise RuntimeError("NGPAdam.reduce_gradients: verdict='poison' needs poison_shards() between the local non-finite sweep and the "
                               "reduce-scatter (step() and graph.GraphedTrainStep issue it); verdict='allreduce' exchanges the verdict itself")
        view = self.flat_grad16.view(self.world_size, self.payload)
        if self._avg_native():
            dist.reduce_scatter_tensor(self.shard_grad, self.flat_grad16, op=dist.ReduceOp.AVG, group=self.group)
        else:  # backends without reduce-scatter / AVG (gloo in the CPU tests): same result through an all-reduce
            self.flat_grad16.mul_(1.0 / self.world_size)
            dist.all_reduce(self.flat_grad16, op=dist.ReduceOp.SUM, group=self.group)
            self.shard_grad.copy_(view[self.rank])
        if self.verdict != 'poison':
            dist.all_reduce(self.scalars.narrow(0, FOUND_INF, 1), op=dist.ReduceOp.MAX, group=self.group)

    def _shard_entries(self):
        """the pieces of parameters inside my shard, as kernel entries"""
        lo, hi = self.shard_range
        out = []
        lr_of = {id(p): g['lr'] for g in self.param_groups for p in g['params']}
        for p, off in zip(self.flat_params, self.offsets):
            a, b = max(off, lo), min(off + p.numel(), hi)
            if a < b:
                out.append(Entry(b - a, self.flat_master[a:b], self.exp_avg[a - lo:b - lo], self.exp_avg_sq[a - lo:b - lo], self.shard_grad[a - lo:b - lo],
                                 self.flat_p16[a:b], 1, lr_of[id(p)], None))
        return out

    @torch.no_grad()
    def apply(self, zero=True):
        """Adam on my shard (skipped everywhere when any rank saw a non-finite gradient), loss-scale / step-count commit, and the flat
        deposit buffer zeroed for the next backward; capturable.  zero=False: the producers of the NEXT step overwrite every element they own
        (the captured fused iteration with overwrite_table: the grid backward writes the whole table gradient, the slab reduction writes the
        MLP gradients), so the 24.5 MB memset is skipped -- the buffers are stale from here on, which a caller that REPLAYS this call has
        to state itself (replayed_kept_deposits) so that a producer that ADDS cleans them first."""
        if len(self._keep) > 64:   # used standalone in a loop without pre_reduce_check()/step(): do not grow without bound
            del self._keep[:-8]
        if self.verdict == 'poison':
            self._verdict_launch()     # element 0 of my averaged shard is NaN when ANY rank flagged its local gradient
        entries = self._shard_entries()
        for i in range(0, len(entries), _MAX):
            self._launch(entries[i:i + _MAX], capi.NGP_OPT_PHASE_UPDATE, 0.0)
        self._launch([], capi.NGP_OPT_PHASE_COMMIT, 0.0)
        if zero:
            self.flat_grad16.zero_()
        if not (self.flat_grad16.is_cuda and torch.cuda.is_current_stream_capturing()):
            self._poisoned = getattr(self, '_poison_captured', False)   # an eager step consumed its poison launch; a captured one replays it
        for p in self.flat_params:   # zeroed: clean, whatever an overwriting producer announced; kept: stale until overwritten / cleaned
            _consumed(p, kept=not zero)

    @torch.no_grad()
    def gather_shadows(self, async_op=True):
        """ONE all-gather of the fp16 shadow weights (every rank contributes its freshly updated shard).  Issued on a side stream after
        the update; `wait_shadows()` makes the consumer's stream wait -- the next iteration's ray marching does not need the weights and
        runs meanwhile."""
        lo, hi = self.shard_range
        mine = self.flat_p16[lo:hi]
        if not (async_op and self.flat_p16.is_cuda):
            self._all_gather(self.flat_p16, mine)
            return
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.flat_p16.device)
            self._shadows_ready = torch.cuda.Event()
        self._comm_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._comm_stream):
            self._all_gather(self.flat_p16, mine)
            self._shadows_ready.record(self._comm_stream)
        self._pending = True

    def _all_gather(self, full, mine):
        if dist.get_backend(self.group) == 'nccl':
            dist.all_gather_into_tensor(full, mine, group=self.group)
        else:
            parts = [torch.empty_like(mine) for _ in range(self.world_size)]
            dist.all_gather(parts, mine.contiguous(), group=self.group)
            full.view(self.world_size, -1).copy_(torch.stack(parts))

    def wait_shadows(self):
        if getattr(self, '_pending', False):
            torch.cuda.current_stream().wait_event(self._shadows_ready)
            self._pending = False

    @torch.no_grad()
    def gather_master(self):
        """complete the fp32 master weights on every rank (each rank only keeps its own shard current): before checkpoints / evaluation
        through the module-by-module path"""
        if self.shard:
            lo, hi = self.shard_range
            self._all_gather(self.flat_master, self.flat_master[lo:hi])

    # -- the step ----------------------------------------------------------------------------------
    def _entries(self, update_ema=None):
        """the `Entry` of every parameter that received a gradient this iteration (with its shadow in `update_ema`, if given).  A parameter
        with neither a `.grad` nor a deposit buffer is left alone, as torch.optim.Adam skips `grad is None` parameters."""
        entries = []
        for g in self.param_groups:
            for p in g['params']:
                st = self.state[p]
                if p.grad is not None:
                    if 'grad16' in st and self._deposit_used(st):
                        raise RuntimeError('NGPAdam: a parameter has BOTH an autograd .grad and a deposited fp16 gradient -- the fused path '
                                           'and the module-by-module path were mixed within one step (or a foreign averager created .grad)')
                    grad, is_half = p.grad, 0
                    if not grad.is_contiguous() or grad.dtype != torch.float32:
                        raise RuntimeError('NGPAdam: p.grad must be a contiguous float32 tensor')
                elif 'grad16' in st:
                    grad, is_half = st['grad16'], 1
                    if getattr(p, '_ngp_deposit_overwritten', False):
                        # this step's producer WROTE the whole buffer (fused iteration with overwrite_table): the update kernel leaves it
                        # alone instead of zeroing it -- it is stale from here on, until the next overwriting producer or a clean_deposits()
                        is_half = 3
                        _consumed(p, kept=True)
                else:
                    continue
                entries.append(Entry(p.numel(), p, st['exp_avg'], st['exp_avg_sq'], grad, st.get('fp16'), is_half, g['lr'],
                                     update_ema.shadow_of(p) if update_ema is not None else None))
        return entries

    clean_deposits = staticmethod(clean_deposits)   # (`optimizer.clean_deposits(params)`: the spelling of graph.py and the tests)

    def _deposit_used(self, st):
        # only checked on the eager path (never while capturing a graph: it reads the device)
        if torch.cuda.is_current_stream_capturing() or not self.check_mixed_gradients:
            return False
        return bool(st['grad16'].ne(0).any().item())

    def _leading_args(self, entries, cast):
        """the arguments both Adam entries start with: count, the first eight arrays of `cast` (_entry_arrays), betas, eps, grad_mult, growth, backoff, interval, state"""
        return [len(entries), *cast[:8], self.betas[0], self.betas[1], self.eps, 1.0, self.growth_factor, self.backoff_factor, self.growth_interval, self.scalars.data_ptr()]

    def _launch(self, entries, phases, omd):
        """one ngp_optim_adam_step_ex call over up to 8 entries (param / moments may be None for a CHECK-only call)"""
        cast = _entry_arrays(entries, omd > 0.0, self._keep)
        capi.check(capi.lib.ngp_optim_adam_step_ex(*self._leading_args(entries, cast), cast[8], float(omd), phases, capi.stream()))

    def _launch_small_commit(self, entries, flip, table_prefix=0):
        ta = self._table_adam_struct() if table_prefix else None   # (copied by the C entry before it returns)
        capi.check(capi.lib.ngp_optim_adam_small_commit(*self._leading_args(entries, _entry_arrays(entries, False, self._keep)), 1 if flip else 0,
                                                        None if ta is None else ctypes.cast(ctypes.pointer(ta), ctypes.c_void_p),
                                                        self.state[self.fused_table]['grad16'].data_ptr() if table_prefix else None, int(table_prefix),
                                                        capi.stream()))

    @torch.no_grad()
    def step(self, update_ema=None, gradients_checked=False):
        """one optimizer + loss-scaling step.  `update_ema`: an `NGPEma` whose moving average is advanced inside the same sweep (the
        Trainer does that once per epoch, nerf/utils.py:760-761,891-892; call it with the last step of the epoch).
        gradients_checked: the kernels that deposited the fp16 gradients already set the FOUND_INF word where a value came out
        non-finite (fused.fused_train_iteration(found_inf=...)), so the sweep of the CHECK phase is not launched; ignored (the sweep runs)
        when any parameter carries an autograd `.grad`.
        Sharded mode: the whole exchange-and-update sequence (pre_reduce_check -> reduce_gradients -> apply -> gather_shadows)."""
        self._keep = []
        CHECK, UPDATE, COMMIT = capi.NGP_OPT_PHASE_CHECK, capi.NGP_OPT_PHASE_UPDATE, capi.NGP_OPT_PHASE_COMMIT
        if self.shard:
            if update_ema is not None:
                raise RuntimeError('NGPAdam(shard=True): fold-in EMA is not available; call gather_master() then ema.update() once per epoch')
            if any(p.grad is not None for p in self.flat_params):
                raise RuntimeError('NGPAdam(shard=True): gradients must be deposited by the fused path (found an autograd .grad)')
            self._refuse_stale_deposits('step')
            if not gradients_checked:
                self.pre_reduce_check()
            self.poison_shards()
            self.reduce_gradients()
            self.apply()
            self.gather_shadows()
            self.wait_shadows()
            return
        table_done = self.fused_table is not None and getattr(self.fused_table, '_ngp_table_adam_done', False)
        if table_done:
            # this step's grid backward already applied Adam to the table (speculatively, into the other buffer set): Adam on the small
            # tensors that are left + commit + parity flip in ONE single-workgroup launch
            self.fused_table._ngp_table_adam_done = False
            if update_ema is not None or not gradients_checked:
                raise RuntimeError('NGPAdam.step: a fused-table step needs gradients_checked=True (the producers raise found_inf) and no fold-in EMA')
            self.clean_deposits([p for p in self.flat_params if p is not self.fused_table and not getattr(p, '_ngp_deposit_overwritten', False)])
            entries = [e for e in self._entries() if e.param is not self.fused_table]
            if len(entries) > _MAX or not all(e.is_half & 1 for e in entries):
                raise RuntimeError('NGPAdam.step: a fused-table step serves at most 8 remaining tensors, all with deposited fp16 gradients')
            # the dense levels at the start of the table (left out by the accumulate's flush) are swept here, contiguously
            prefix = int(getattr(self.fused_table, '_ngp_table_adam_prefix', 0)) * int(self.fused_table.shape[1])
            self._launch_small_commit(entries, flip=True, table_prefix=prefix)
            return
        self.materialize()   # (a no-op unless fused-table steps ran before this unfused one)
        # a deposit buffer that an overwriting producer left behind and nobody has overwritten since holds an OLD gradient
        self.clean_deposits([p for p in self.flat_params if not getattr(p, '_ngp_deposit_overwritten', False)])
        omd = update_ema.begin_update() if update_ema is not None else 0.0
        entries = self._entries(update_ema)
        chunks = [entries[i:i + _MAX] for i in range(0, len(entries), _MAX)]
        checked = gradients_checked and all(e.is_half & 1 for e in entries)   # every gradient is a deposited fp16 buffer
        if len(chunks) == 1:
            self._launch(chunks[0], (0 if checked else CHECK) | UPDATE | COMMIT, omd)
        else:
            # "skipped as a whole": every chunk is swept for non-finite values BEFORE any chunk is updated (GradScaler.step semantics)
            for c in ([] if checked else chunks):
                self._launch(c, CHECK, 0.0)
            for c in chunks:
                self._launch(c, UPDATE, omd)
            self._launch([], COMMIT, 0.0)

    # -- checkpointing -----------------------------------------------------------------------------
    def load_torch_adam_state(self, adam_sd, scaler_sd=None):
        """resume from a reference checkpoint: `torch.optim.Adam.state_dict()` (per-parameter exp_avg / exp_avg_sq / step, in
        param_groups order) and, optionally, `GradScaler.state_dict()` ('scale', '_growth_tracker')"""
        flat = [p for g in self.param_groups for p in g['params']]
        self.materialize()
        ids = [i for g in adam_sd['param_groups'] for i in g['params']]
        if len(ids) != len(flat):
            raise RuntimeError(f'NGPAdam: checkpoint has {len(ids)} parameters, the optimizer {len(flat)}')
        step = 0.0
        for p, i in zip(flat, ids):
            st = adam_sd['state'].get(i)
            if st is None:
                continue
            self._set_moments(p, st['exp_avg'], st['exp_avg_sq'])
            step = max(step, float(st['step']))
        self.scalars.narrow(0, STEP_COUNT, 1).fill_(step)
        # learning rate: the group keeps the scheduler-free base rate, the scheduler's current factor (LambdaLR writes lr =
        # initial_lr * lambda(step), main_nerf.py:137) goes into the device-side multiplier -- a resumed run continues at the decayed rate
        factors = []
        for g, tg in zip(self.param_groups, adam_sd['param_groups']):
            base = float(tg.get('initial_lr', tg['lr']))
            g['lr'] = base
            factors.append(float(tg['lr']) / base if base != 0.0 else 1.0)
        if factors:
            if max(factors) - min(factors) > 1e-6 * max(1.0, max(factors)):
                # per-group schedules: fold each factor into its group's rate, keep the common multiplier at 1
                for g, f in zip(self.param_groups, factors):
                    g['lr'] *= f
                self.set_lr_scale(1.0)
            else:
                self.set_lr_scale(factors[0])
        if scaler_sd:
            self.scalars.narrow(0, SCALE, 1).fill_(float(scaler_sd.get('scale', self.get_scale())))
            self.scalars.narrow(0, GROWTH_TRACKER, 1).fill_(float(scaler_sd.get('_growth_tracker', 0)))
        self._sync_shadows(assume_complete=True)   # the caller loaded the full parameter set on every rank

    def _shard_piece(self, p):
        """(a, b, off): the packed range [a, b) of parameter p inside my shard (a >= b: nothing) and p's packed offset"""
        off = self.offsets[[id(q) for q in self.flat_params].index(id(p))]
        lo, hi = self.shard_range
        return max(off, lo), min(off + p.numel(), hi), off

    def _set_moments(self, p, m, v):
        if not self.shard:
            self.state[p]['exp_avg'].copy_(m)
            self.state[p]['exp_avg_sq'].copy_(v)
            return
        a, b, off = self._shard_piece(p)
        if a < b:
            lo = self.shard_range[0]
            self.exp_avg[a - lo:b - lo].copy_(m.reshape(-1)[a - off:b - off])
            self.exp_avg_sq[a - lo:b - lo].copy_(v.reshape(-1)[a - off:b - off])

    def _get_moments(self, p):
        if not self.shard:
            return self.state[p]['exp_avg'].clone(), self.state[p]['exp_avg_sq'].clone()
        m, v = torch.zeros_like(p).reshape(-1), torch.zeros_like(p).reshape(-1)
        a, b, off = self._shard_piece(p)
        if a < b:
            lo = self.shard_range[0]
            m[a - off:b - off].copy_(self.exp_avg[a - lo:b - lo])
            v[a - off:b - off].copy_(self.exp_avg_sq[a - lo:b - lo])
        dist.all_reduce(m, group=self.group)  # every element is owned by exactly one rank: the sum assembles the full tensor
        dist.all_reduce(v, group=self.group)
        return m.view_as(p), v.view_as(p)

    def state_dict(self):
        """full (unsharded) optimizer state; in sharded mode a collective call (every rank assembles the complete moments)"""
        flat = [p for g in self.param_groups for p in g['params']]
        self.materialize()
        if self.shard:
            self.gather_master()
        mv = [self._get_moments(p) for p in flat]
        return {'scalars': self.scalars.clone(), 'exp_avg': [m for m, _ in mv], 'exp_avg_sq': [v for _, v in mv],
                'lr': [g['lr'] for g in self.param_groups]}

    def load_state_dict(self, sd):
        flat = [p for g in self.param_groups for p in g['params']]
        self.materialize()
        self.scalars.copy_(sd['scalars'])
        self.scalars.narrow(0, TABLE_PARITY, 1).zero_()   # (the parity of a fused table is not part of a checkpoint: set A is what gets loaded)
        for p, m, v in zip(flat, sd['exp_avg'], sd['exp_avg_sq']):
            self._set_moments(p, m, v)
        for g, lr in zip(self.param_groups, sd['lr']):
            g['lr'] = lr
        self._sync_shadows(assume_complete=True)   # load_state_dict follows model.load_state_dict on every rank (checkpoint.py)


class NGPEma:
    """Exponential moving average of the parameters with torch_ema.ExponentialMovingAverage's surface and update rule (the reference
    Trainer's `self.ema`, nerf/utils.py:388-391: update() once per epoch :760-761,891-892, store()/copy_to()/restore() around evaluation
    :800-810,928-1011, state_dict() in checkpoints :1034-1035):

        decay_t = min(decay, (1 + num_updates) / (10 + num_updates))          (use_num_updates=True, torch_ema's default)
        shadow -= (1 - decay_t) * (shadow - param)

    `update()` is one fused launch over all parameters (ngp_optim_ema_update); `NGPAdam.step(update_ema=ema)` folds it into the Adam
    sweep instead.  copy_to()/restore() refresh the optimizer's fp16 shadow weights when given the optimizer."""

    def __init__(self, parameters, decay, use_num_updates=True, optimizer=None):
        if decay < 0.0 or decay > 1.0:
            raise ValueError('Decay must be between 0 and 1')
        self.params = [p for p in parameters if p.requires_grad]
        self.decay = float(decay)
        self.num_updates = 0 if use_num_updates else None
        self.optimizer = optimizer
        self._complete_params()
        self.shadow_params = [p.detach().clone() for p in self.params]
        self.collected_params = None
        self._index = {id(p): i for i, p in enumerate(self.params)}

    def shadow_of(self, p):
        return self.shadow_params[self._index[id(p)]]

    def begin_update(self):
        """advance the update counter and return this update's (1 - decay_t)"""
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        return 1.0 - decay

    def _complete_params(self):
        """sharded optimizer: the fp32 parameters this rank does not own are stale between steps -- complete them first (collective)"""
        opt = self.optimizer
        if opt is not None and hasattr(opt, 'materialize'):
            opt.materialize()   # a table with two buffer sets (enable_table_fusion): the torch Parameter becomes the current one
        if opt is not None and getattr(opt, 'shard', False):
            opt.wait_shadows()
            opt.gather_master()

    @torch.no_grad()
    def update(self):
        self._complete_params()
        omd = self.begin_update()
        self._keep = []
        for i in range(0, len(self.params), _MAX):
            entries = [Entry(p.numel(), p, None, None, None, None, 0, 0.0, t) for p, t in zip(self.params[i:i + _MAX], self.shadow_params[i:i + _MAX])]
            cast = _entry_arrays(entries, True, self._keep)
            capi.check(capi.lib.ngp_optim_ema_update(len(entries), cast[0], cast[1], cast[8], float(omd), capi.stream()))

    @torch.no_grad()
    def copy_to(self):
        if self.optimizer is not None and hasattr(self.optimizer, 'materialize'):
            self.optimizer.materialize()   # BEFORE the parameters are written (else the sync below would copy set B over them)
        for s_, p in zip(self.shadow_params, self.params):
            p.copy_(s_)  # bumps the version counter: stale fp16 shadows are detected by resync_stale_shadows
        if self.optimizer is not None:
            self.optimizer._sync_shadows(assume_complete=True)   # every rank just wrote the complete parameter set

    @torch.no_grad()
    def store(self):
        self._complete_params()
        self.collected_params = [p.detach().clone() for p in self.params]

    @torch.no_grad()
    def restore(self):
        if self.collected_params is None:
            raise RuntimeError('This ExponentialMovingAverage has no `store()`ed weights to `restore()`')
        if self.optimizer is not None and hasattr(self.optimizer, 'materialize'):
            self.optimizer.materialize()
        for c, p in zip(self.collected_params, self.params):
            p.copy_(c)
        if self.optimizer is not None:
            self.optimizer._sync_shadows(assume_complete=True)

    def state_dict(self):
        return {'decay': self.decay, 'num_updates': self.num_updates, 'shadow_params': self.shadow_params,
                'collected_params': self.collected_params}

    def load_state_dict(self, sd):
        self.decay = float(sd['decay'])
        self.num_updates = sd['num_updates']
        for s_, t in zip(self.shadow_params, sd['shadow_params']):
            s_.copy_(t)
        cp = sd.get('collected_params')
        self.collected_params = None if cp is None else [t.detach().clone().to(p.device) for t, p in zip(cp, self.params)]
