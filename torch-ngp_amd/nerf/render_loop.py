"""The eval frame of NeRFRenderer.run_cuda with its loop state on the device (extension; DESIGN.md 3.2 has the reasons and the measurements).

The alive count, the per-iteration n_step = clamp(n_total // n_alive, 1, cap) and the marched-step total live in a device word pair that
the march / composite / compaction kernels read, so the host issues several iterations back to back and reads the count back once per
batch.  Between read-backs the launches are sized for the last count read; lanes and sample rows beyond the true count do nothing / are
zero rows.  A ray's samples and their compositing order do not depend on how they are chunked into iterations: same image as the
host-driven loop, bit for bit (tests/test_gpu_pipeline.py).

LoopOptions  every knob of the loop, read once per frame
Schedule     the host's policy -- how many iterations to issue until the next read-back, and with which lanes / rows / n_total / cap --
             as plain Python (no torch, no native library: tests/test_render_loop_schedule.py runs it on the CPU)
FrameLoop    the frame's buffers, the seeding of the alive list, the issuers of an iteration pair and the loop over the schedule

k_march_rays writes n_alive * n_step rows without looking at the buffer's size and k_composite_rays / k_compact_* trust `lanes`, so every
batch of the schedule must hold, for every alive count a the device may reach before the next read-back (1 <= a <= bound_alive):
a * loop_n_step(n_total, a, cap) <= rows and a <= lanes (checked over the schedule's whole domain by the CPU test).
"""
import os
from collections import namedtuple


class LoopOptions:
    """the loop's knobs, attributes of the model unless noted (name: default), each read once per frame:
    graph_loop: False        replay the pairs after the first from HIP graphs, one per row bucket (fixed reference n_step rule: switches
                             `adaptive` off and the tail cap to 8); not after a failed capture (graphs_failed), not with aux_infer
    cull_empty_rays: True    leave rays that meet no occupied voxel out of the first alive list; not with perturb (the start offsets are
                             drawn per alive-list SLOT) and only where k_cull_rays applies (power-of-two grid >= 16; FrameLoop: backend has it)
    adaptive_n_step: True    the adaptive row budget (Schedule.next)
    loop_tail_cap: 64        the cap of samples per ray and iteration once few rays survive, 8..1024; the attribute, when set, wins over the
                             environment's NGP_LOOP_TAIL_CAP
    loop_initial_boost: 2    row budget of the first pair in multiples of the ray count; NGP_LOOP_INITIAL_BOOST, when set, wins over the
                             attribute; 1 with perturb (the first call's samples are the offset ones: their number must follow the reference's rule)
    loop_max_rows: 1 << 26   no boost beyond this many rows
    native_loop: True        one ngp_render_iterations_dev call per pair -- a Python callable cannot be issued from C (aux_infer), and nobody
                             may be probing the stages; FrameLoop also needs the entry in the library and fused.inference_weights; not for a
                             model with takes_deltas (it is called as model(xyzs, dirs, deltas=deltas), per stage)
    loop_device_rows: True   the native call's march publishes the rows that carry a sample; encoder and network stop there
    _loop_probe: None        a list: (stage, start event, end event, lanes, rows, n_total, state snapshot) per stage of every iteration
    _loop_iter_hook: None    called with every iteration's deltas
    _loop_debug: None        a list: (iterations done, alive bound, boost, survival per iteration) at every read-back
    A knob that is not set costs ~1 us through nn.Module.__getattr__, and what the host does in front of the frame's first launch is added
    to the frame: the constructor reads the two knobs the buffers and the seeding depend on, read_policy() the others -- FrameLoop calls it
    with the culling kernels in flight."""

    def __init__(self, model, perturb=False, aux_infer=None, sync_every=8, graphs_failed=False):
        self.model, self.perturb, self.aux_infer, self.sync_every = model, perturb, aux_infer, sync_every
        self.graphs = bool(getattr(model, 'graph_loop', False)) and not graphs_failed and aux_infer is None
        grid = model.grid_size
        self.cull = bool(getattr(model, 'cull_empty_rays', True)) and not perturb and grid >= 16 and (grid & (grid - 1)) == 0

    def read_policy(self):
        model = self.model
        self.probe, self.iter_hook = getattr(model, '_loop_probe', None), getattr(model, '_loop_iter_hook', None)
        self.debug = getattr(model, '_loop_debug', None)
        self.adaptive = bool(getattr(model, 'adaptive_n_step', True)) and not self.graphs
        tail_cap = int(getattr(model, 'loop_tail_cap', os.environ.get('NGP_LOOP_TAIL_CAP', 64))) if self.adaptive else 8
        self.tail_cap = max(8, min(tail_cap, 1024))
        self.initial_boost = 1 if self.perturb else max(1, int(os.environ.get('NGP_LOOP_INITIAL_BOOST', getattr(model, 'loop_initial_boost', 2))))
        self.max_rows = int(getattr(model, 'loop_max_rows', 1 << 26))
        self.scaled = hasattr(model, 'forward_scaled')   # (the fused network folds the density scale: one launch less per iteration)
        self.takes_deltas = bool(getattr(model, 'takes_deltas', False))   # (an SDF model: called with the iteration's deltas, stage by stage)
        self.native = (bool(getattr(model, 'native_loop', True)) and self.aux_infer is None and self.probe is None and self.iter_hook is None
                       and self.scaled and not self.takes_deltas)
        self.device_rows = bool(getattr(model, 'loop_device_rows', True))
        return self


# what to issue until the next read-back: `pairs` times an iteration pair of these launch arguments (cap 0: the kernels' 8); bucket: the
# row bucket a captured pair is kept under; debug: the `_loop_debug` tuple of the read-back
Batch = namedtuple('Batch', 'pairs lanes rows n_total cap bucket debug')


class Schedule:
    """The row budget and the batch sizes of one frame.  The reference marches n_step = clamp(N // n_alive, 1, 8), about N rows per
    iteration; here n_total = boost x N rows and a cap of up to `tail_cap`:
    - boost doubles (up to 8) from the 6th iteration on while at least 9 of 10 rays survive an iteration -- every march call walks the
      surviving rays to the far plane however few samples it emits -- and halves when fewer than 3 of 4 do;
    - the cap is lifted to N // alive (8..tail_cap) once the survivors are few, so that an iteration still evaluates about N rows;
    - batches grow 2, 2, 4, 8, 8, ... iterations; in the tail (alive <= N / 16) the host looks after every pair (two with device-side row
      counts, where a nearly empty iteration is cheaper than a read-back).
    The loop ends when the SUM of iterations reaches max_steps, as the reference's does with its own n_step sequence: a ray that is
    still alive then is truncated at a different sample (only reachable by a ray that itself needs >= max_steps samples);
    adaptive_n_step = False, loop_tail_cap = 8 and loop_initial_boost = 1 give the reference's sequence.
    `pad` is the marchers' padding rule (raymarching._round_up_strict to 128: the fused network wants multiples of 128)."""

    def __init__(self, n_rays, max_steps, opt, pad):
        self.n_rays, self.max_steps, self.opt, self.pad = n_rays, max_steps, opt, pad
        self.graphs = opt.graphs
        self.done, self.batch, self.boost, self.prev_alive, self.prev_iters = 0, 2, 1, n_rays, 2

    def first(self):
        """the first pair: full-frame sized, kernel-bound, the only one that may perturb"""
        n_total = self.opt.initial_boost * self.n_rays
        self.done = 2
        return Batch(1, self.n_rays, self.pad(n_total), n_total, 0, n_total, None)

    def capture_failed(self):
        """the rest of the frame is issued eagerly (the batch in hand keeps its bucket-sized rows and lanes)"""
        self.graphs = False

    def next(self, bound_alive, device_rows):
        """the batch behind a read-back of `bound_alive` rays, None when the frame is over"""
        opt, n_rays = self.opt, self.n_rays
        if bound_alive <= 0 or self.done >= self.max_steps:
            return None
        if self.done > 2 and opt.adaptive and opt.tail_cap > 8 and bound_alive * 16 <= n_rays:
            # the tail: a pair now marches up to 2 x cap samples per ray -- look before launching more
            self.batch = 4 if device_rows else 2
        cap = max(8, min(opt.tail_cap, n_rays // bound_alive))
        survival = None
        if opt.adaptive:
            survival = (bound_alive / max(self.prev_alive, 1)) ** (1.0 / max(self.prev_iters, 1))
            if survival >= 0.9 and self.boost < 8 and self.done >= 6 and 2 * self.boost * n_rays <= opt.max_rows:
                self.boost *= 2
            elif survival < 0.75 and self.boost > 1:
                self.boost //= 2
            survival = round(survival, 3)
        n_total = self.boost * n_rays
        debug = (self.done, bound_alive, self.boost, survival)
        # row bucket: the smallest of B, B/2, B/4, ... (B = n_total) that holds min(B, cap * alive) rows (>= 2048).  Buckets exist for the
        # graphs, one captured pair each; without graphs the buffers are sized exactly
        need = min(n_total, cap * bound_alive)
        bucket = n_total
        while bucket // 2 >= max(need, 2048):
            bucket //= 2
        if self.graphs:
            rows, lanes = self.pad(bucket), n_rays if bucket == n_rays else bucket // 8 + 1
        else:
            rows, lanes = self.pad(need), min(n_rays, bound_alive)
        pairs = max(1, self.batch // 2)
        self.prev_alive, self.prev_iters = bound_alive, 2 * pairs
        self.done += 2 * pairs
        self.batch = min(opt.sync_every, self.batch * 2) if self.done >= 6 else (4 if device_rows else self.batch)
        return Batch(pairs, lanes, rows, n_total, 0 if cap == 8 else cap, bucket, debug)


def _cache(model, tensors, dt_gamma, max_steps, T_thresh, capi):
    """the loop's buffers, kept on the model (`_loop_cache`) while frames of the same shape and settings follow each other"""
    import torch
    rays_o = tensors[0]
    n_rays, dev = rays_o.shape[0], rays_o.device
    key = (n_rays, str(dev), float(dt_gamma), int(max_steps), float(T_thresh), float(model.density_scale), model.density_bitfield.data_ptr(),
           torch.is_autocast_enabled('cuda'), model.training)
    cache = getattr(model, '_loop_cache', None)
    if cache is None or cache['key'] != key:
        cache = {'key': key, 'graphs': {}, 'failed': False,
                 'alive': [torch.empty(n_rays, dtype=torch.int32, device=dev), torch.empty(n_rays, dtype=torch.int32, device=dev)],
                 'state': torch.zeros(2, 2, dtype=torch.int32, device=dev),
                 'ws': torch.empty(int(capi.lib.ngp_compact_rays_workspace_bytes(n_rays)), dtype=torch.uint8, device=dev),
                 'bufs': [torch.empty_like(t) for t in tensors],
                 'arange': torch.arange(n_rays, dtype=torch.int32, device=dev)}
        model._loop_cache = cache
    return cache


class StageIssuer:
    """an iteration as one Python call per stage (ten calls and six allocations per pair); `probe`: HIP events around every stage"""

    def __init__(self, frame):
        from raymarching import backend as rf   # (the feature compositor's entries are ctypes-only)
        self.f, self.rf, self.probe, self.tag = frame, rf, frame.opt.probe, None

    def stage(self, name, fn):
        if self.probe is None:
            return fn()
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.probe.append((name, e0, e1) + self.tag)
        return out

    def iteration(self, cur, lanes, rows, noises, n_total, cap):
        import torch
        f, m, stage = self.f, self.f.model, self.stage
        rb, state, alive, T_thresh = f.rb, f.state[cur], f.alive[cur], f.T_thresh
        if self.probe is not None:
            self.tag = (lanes, rows, n_total, state.clone())
        xyzs, dirs, deltas = (torch.empty(rows, width, dtype=torch.float32, device=f.dev) for width in (3, 3, 2))
        stage('march_rays', lambda: rb.march_rays_dev(state, lanes, n_total, cap, alive, f.t, f.o, f.d, m.bound, f.dt_gamma, f.max_steps, m.cascade,
                                                      m.grid_size, f.bits, f.near, f.far, xyzs, dirs, deltas, noises, rows))
        if f.opt.iter_hook is not None:
            f.opt.iter_hook(deltas)
        scaled = f.opt.scaled and not f.opt.takes_deltas
        sigmas, rgbs = stage('network (encoder + MLPs + glue)', lambda: m.forward_scaled(xyzs, dirs, m.density_scale) if scaled else
                             m(xyzs, dirs, deltas=deltas) if f.opt.takes_deltas else m(xyzs, dirs))
        sigmas, rgbs32 = stage('casts (density_scale, fp32 copies)', lambda: ((sigmas if scaled else m.density_scale * sigmas).float().contiguous(),
                                                                               rgbs.float().contiguous()))
        if f.aux_infer is not None:   # before composite_rays_dev: the feature kernel reads the weights_sum that call advances
            feats = stage('aux_infer (the caller\'s channels)', lambda: m._aux_infer_feats(f.aux_infer, f.aux_frame, xyzs, dirs, sigmas, rgbs32, f.n_rays))
            stage('composite_rays_features', lambda: self.rf.composite_rays_features_dev(state, lanes, n_total, cap, T_thresh, alive, sigmas, feats, deltas,
                                                                                         f.weights_sum, f.aux_frame['out']))
        stage('composite_rays', lambda: rb.composite_rays_dev(state, lanes, n_total, cap, T_thresh, alive, f.t, sigmas, rgbs32, deltas, f.weights_sum,
                                                              f.depth, f.image))
        stage('compact_rays', lambda: rb.compact_rays_dev(state, lanes, n_total, cap, f.max_steps, alive, f.alive[1 - cur], f.state[1 - cur], f.ws))

    def pair(self, lanes, rows, noises, n_total, cap):
        """iterations on state 0 then state 1"""
        self.iteration(0, lanes, rows, noises, n_total, cap)
        self.iteration(1, lanes, rows, None, n_total, cap)


class NativeIssuer:
    """an iteration pair as ONE ngp_render_iterations_dev call: the same kernels, arguments and order as StageIssuer's, issued from C"""

    def __init__(self, frame, weights):
        import ctypes
        import fused
        f, m, capi = frame, frame.model, frame.capi
        emb16, ws16, wc16, cfg = weights
        a = capi.RenderLoop()
        a.state, a.alive[0], a.alive[1] = f.state.data_ptr(), f.alive[0].data_ptr(), f.alive[1].data_ptr()
        a.rays_t, a.rays_o, a.rays_d, a.nears, a.fars, a.grid = (t.data_ptr() for t in (f.t, f.o, f.d, f.near, f.far, f.bits))
        a.embeddings, a.offsets, a.w_sigma, a.w_color = emb16.data_ptr(), m.encoder.offsets.data_ptr(), ws16.data_ptr(), wc16.data_ptr()
        a.level_cost_host = capi.ray_level_costs(cfg.L, cfg.S, cfg.H, 3.0 ** 0.5 / (1024.0 * max(float(cfg.bound), 1e-6))) if fused.USE_BALANCED_FORWARD else None
        a.weights_sum, a.depth, a.image, a.compact_workspace = f.weights_sum.data_ptr(), f.depth.data_ptr(), f.image.data_ptr(), f.ws.data_ptr()
        a.max_steps, a.cascade, a.grid_size = int(f.max_steps), int(m.cascade), int(m.grid_size)
        a.L, a.H, a.gridtype, a.interp, a.num_layers_sigma, a.num_layers_color = cfg.L, cfg.H, cfg.gridtype, cfg.interp, cfg.nl_sigma, cfg.nl_color
        a.align_corners = cfg.align
        a.bound, a.dt_gamma, a.T_thresh, a.S, a.density_scale = float(m.bound), float(f.dt_gamma), float(f.T_thresh), float(cfg.S), float(m.density_scale)
        if f.opt.device_rows:
            if 'rows_used' not in f.cache:
                import torch
                f.cache['rows_used'] = torch.zeros(1, dtype=torch.int32, device=f.dev)
            a.rows_used = f.cache['rows_used'].data_ptr()
        self.f, self.args, self.args_ptr, self.call = f, a, ctypes.cast(ctypes.pointer(a), ctypes.c_void_p), capi.lib.ngp_render_iterations_dev
        # kept alive until the frame is over (the launches are asynchronous): the fp16 weights, every pair's noises and the sample buffers --
        # ONE block per frame, re-made only when a pair needs more rows than any before it (the first pair is the largest of an opaque frame)
        self.weights, self.noises, self.rows, self.samples = (emb16, ws16, wc16), [], 0, None

    def pair(self, lanes, rows, noises, n_total, cap):
        a, m, capi = self.args, self.f.model, self.f.capi
        if self.rows < rows:
            import torch
            f32 = dict(dtype=torch.float32, device=self.f.dev)
            self.samples = (torch.empty(rows, 3, **f32), torch.empty(rows, 3, **f32), torch.empty(rows, 2, **f32),
                            torch.empty(a.L * rows * 2, dtype=torch.half, device=self.f.dev), torch.empty(rows, **f32), torch.empty(rows, 3, **f32))
            self.rows = rows
            a.xyzs, a.dirs, a.deltas, a.enc, a.sigmas, a.rgbs = [t.data_ptr() for t in self.samples]
        self.noises.append(noises)
        a.noises = None if noises is None else noises.data_ptr()
        a.lanes, a.rows, a.n_total, a.n_step_cap = int(lanes), int(rows), int(n_total), int(cap)
        capi.check(self.call(self.args_ptr, 2, 0, capi.stream()))
        m._loop_native_pairs = getattr(m, '_loop_native_pairs', 0) + 1


class FrameLoop:
    """one eval frame: tensors = (rays_o, rays_d, nears, fars, rays_t, weights_sum, depth, image), the last three accumulated in place.
    aux_infer / aux_frame (run_cuda): the caller's channels, composited into aux_frame['out'] in front of every composite."""

    def __init__(self, model, tensors, perturb, dt_gamma, max_steps, T_thresh, sync_every=8, aux_infer=None, aux_frame=None):
        from raymarching.raymarching import _backend as rb, _round_up_strict   # compiled binding when built, else ctypes (same C ABI)
        import _ngp_capi as capi
        self.model, self.rb, self.capi = model, rb, capi
        self.n_rays, self.dev = tensors[0].shape[0], tensors[0].device
        self.dt_gamma, self.max_steps, self.T_thresh, self.aux_infer, self.aux_frame = dt_gamma, max_steps, T_thresh, aux_infer, aux_frame
        cache = self.cache = _cache(model, tensors, dt_gamma, max_steps, T_thresh, capi)
        opt = self.opt = LoopOptions(model, perturb, aux_infer, sync_every, graphs_failed=cache['failed'])
        # static buffers (the graphs hold their addresses, and the accumulators must be updated in place): this frame's inputs and
        # accumulators are copied in, the results copied out; otherwise the loop works on the caller's tensors
        frame = tuple(t.contiguous() for t in tensors)
        self.results = tensors[5:]
        self.static = opt.graphs or any(a is not b for a, b in zip(frame[5:], self.results))
        if self.static:
            for dst, src in zip(cache['bufs'], tensors):
                dst.copy_(src)
            frame = cache['bufs']
        self.o, self.d, self.near, self.far, self.t, self.weights_sum, self.depth, self.image = frame
        self.alive, self.state, self.ws = cache['alive'], cache['state'], cache['ws']
        self.bits, self.pad = model.density_bitfield.contiguous(), lambda rows: _round_up_strict(rows, 128)

    def seed(self):
        """the first alive list: every ray, or the rays k_cull_rays cannot rule out -- conservatively, from a dilated (H/4)^3 occupancy per
        cascade: the others would have produced no sample"""
        import torch
        m, rb, cache, n_rays = self.model, self.rb, self.cache, self.n_rays
        self.state.zero_()
        if not (self.opt.cull and hasattr(rb, 'cull_rays')):
            self.alive[0].copy_(cache['arange'])
            self.state[0, 0] = n_rays
            return
        if cache.get('coarse') is None:
            cache['coarse'] = torch.empty(int(self.capi.lib.ngp_coarse_occupancy_bytes(m.cascade, m.grid_size)), dtype=torch.uint8, device=self.dev)
            cache['flags'] = torch.empty(n_rays, dtype=torch.int32, device=self.dev)
        rb.coarse_occupancy(self.bits, m.cascade, m.grid_size, cache['coarse'])
        rb.cull_rays(self.o, self.d, self.near, self.far, n_rays, float(m.bound), m.cascade, m.grid_size, cache['coarse'], cache['flags'])
        rb.compact_rays(cache['flags'], n_rays, self.alive[0], self.state[0])     # state[0] = {rays kept, 0 steps marched}

    def graph(self, batch, schedule):
        """the captured pair of the batch's row bucket (captured on first use, kept on the model); None after a capture that failed: the
        frame goes on eagerly and the caller can inspect _loop_cache['failed']"""
        import torch
        g = self.cache['graphs'].get(batch.bucket)
        if g is None:
            try:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):   # (two per-stage iterations, also where the eager pairs are native)
                    StageIssuer(self).pair(batch.lanes, batch.rows, None, batch.n_total, batch.cap)
                self.cache['graphs'][batch.bucket] = g
            except Exception as e:  # noqa: BLE001
                self.cache['failed'] = repr(e)
                schedule.capture_failed()
                g = None
                torch.cuda.synchronize()
        return g

    def run(self):
        import torch
        # the host work in front of the first launches is added to the frame, the work behind them is not: seed first, then read the
        # policy knobs and build the schedule and the native argument block while the culling kernels run
        self.seed()
        opt, state = self.opt.read_policy(), self.state
        schedule = Schedule(self.n_rays, self.max_steps, opt, self.pad)
        # the issuers hold the frame, the frame does not hold them: everything (the native issuer's sample buffers too) is released when
        # the frame is over, without waiting for the cycle collector
        weights = None
        if opt.native and hasattr(self.capi.lib, 'ngp_render_iterations_dev'):
            import fused
            weights = fused.inference_weights(self.model, self.o)   # (None unless the network call would run the fused path on pinned fp16 weights)
        issuer = StageIssuer(self) if weights is None else NativeIssuer(self, weights)
        device_rows = weights is not None and opt.device_rows
        noises = torch.rand(self.n_rays, dtype=torch.float32, device=self.dev) if opt.perturb else None
        batch = schedule.first()
        issuer.pair(batch.lanes, batch.rows, noises, batch.n_total, batch.cap)
        for batch in iter(lambda: schedule.next(int(state[0, 0].item()), device_rows), None):   # one read-back per batch
            if opt.debug is not None:
                opt.debug.append(batch.debug)
            g = self.graph(batch, schedule) if schedule.graphs else None
            for _ in range(batch.pairs):
                if g is not None:
                    g.replay()
                else:
                    issuer.pair(batch.lanes, batch.rows, None, batch.n_total, batch.cap)
        if self.static:
            for dst, src in zip(self.results, (self.weights_sum, self.depth, self.image)):
                dst.copy_(src)
