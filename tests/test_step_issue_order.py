"""CPU: what graph.GraphedTrainStep issues, on which stream and in which order, in every replay shape -- pinned against a golden log
(tests/golden/step_issue_order.json) that was produced by the module as it stood BEFORE its records-and-shapes restructuring and is not
regenerated from later code.

Nothing of the device is needed: the stepper is driven through its public entry points (`precapture`, `step`, `close`) over doubles at its
outer boundaries only -- torch.cuda's graphs, pools, streams and events, the two fused iteration entries, cmdlist.CommandList, the
optimizer, the model and optim's two replay marks.  A stub graph is named after what ran inside its capture and the capacity it was
captured for (`march0@24576`); a replay logs `<current stream>:replay(<graph>)`.  Copies are checked by value: batch k holds rays_o = k,
rays_d = k + 0.25, target = k + 0.5, and every step logs which static buffer holds which batch, the lookahead's seed words and the
model's sample-count ring (counter row p holds 100 + p)."""
import contextlib
import json
import os

import pytest
import torch

N = 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_issue_order.json')
LIST_NAMES = ['k_grid_forward_fast', 'k_network_forward', 'k_composite_train_loss_bwd', 'k_grid_backward_bin', 'k_grid_backward_accumulate',
              'k_adam_small_commit']


class _Harness:
    """the log, the stream stack and the capture in progress"""

    def __init__(self):
        self.log, self.streams, self.capturing, self.recording = [], [_Stream(self, 'main')], None, None
        self.n_streams = self.n_events = self.n_pools = self.n_graphs = 0
        self.fail_graph_at = None      # the CUDAGraph() construction (counted from 0) that raises

    def op(self, name):
        """something that launches: inside a capture it becomes part of the graph's (and the recording list's) name, else it is logged"""
        if self.capturing is not None:
            self.capturing.ops.append(name)
        else:
            self.log.append(f'{self.streams[-1].name}:{name}')

    def take(self):
        out, self.log = self.log, []
        return out


class _Stream:
    def __init__(self, h, name):
        self.h, self.name, self.cuda_stream = h, name, name

    def wait_event(self, e):
        self.h.log.append(f'{self.name}.wait_event({e.name})')

    def wait_stream(self, s):
        self.h.log.append(f'{self.name}.wait_stream({s.name})')

    def synchronize(self):
        self.h.log.append(f'{self.name}.synchronize')


class _Graph:
    def __init__(self, h):
        if h.fail_graph_at is not None and h.n_graphs >= h.fail_graph_at:
            raise RuntimeError('stub: the graph cannot be created')
        h.n_graphs += 1
        self.h, self.ops, self.cap, self._pool = h, [], None, None

    @property
    def name(self):
        return '+'.join(self.ops) + (f'@{self.cap}' if self.cap else '')

    def pool(self):
        return self._pool

    def replay(self):
        self.h.log.append(f'{self.h.streams[-1].name}:replay({self.name})')


class _List:
    """cmdlist.CommandList: entered inside the capture whose chain it records"""

    def __init__(self, h):
        self.h, self.graph, self.handle = h, None, 1

    def __enter__(self):
        self.graph = self.h.capturing
        return self

    def __exit__(self, *exc):
        return False

    def names(self):
        return list(LIST_NAMES)

    def mark(self, mark_id, index):
        self.h.log.append(f'list({self.graph.name}).mark({mark_id},{index})')

    def replay(self, stream):
        self.h.log.append(f'{stream}:list.replay({self.graph.name})')

    def wait_mark(self, mark_id, stream):
        self.h.log.append(f'list({self.graph.name}).wait_mark({mark_id},{stream})')

    def destroy(self):
        if self.handle is not None:   # (as cmdlist.CommandList: destroying a destroyed list does nothing)
            self.h.log.append(f'list({self.graph.name}).destroy')
            self.handle = None


class _Opt:
    """the optimizer as the stepper sees it (optim.NGPAdam's surface: it owns the loss scale and deposits gradients)"""

    def __init__(self, h, params, shard=False, table_fusion=False):
        self.h, self.flat_params, self.shard = h, params, shard
        self.flat_grad16, self.scalars = torch.zeros(4, dtype=torch.half), torch.zeros(8)
        if table_fusion:
            self.enable_table_fusion = lambda emb: h.op('opt.enable_table_fusion')

    def scale(self, loss):
        return loss

    def zero_grad(self, set_to_none=True):
        self.h.op('zero')

    def step(self, gradients_checked=False):
        self.h.op('step_checked' if gradients_checked else 'step')

    def apply(self, zero=True):
        self.h.op(f'apply(zero={zero})')

    def gather_shadows(self, async_op=True):
        self.h.op('gather_shadows' if async_op else 'gather_shadows(sync)')

    def clean_deposits(self, params):
        self.h.op(f'clean_deposits({len(params)})')


for _name in ('wait_shadows', 'reduce_gradients', 'all_reduce', 'pre_reduce_check', 'poison_shards', 'captures_discarded', 'materialize'):
    setattr(_Opt, _name, (lambda n: lambda self: self.h.op(n))(_name))


class _Model(torch.nn.Module):
    def __init__(self, h, table):
        super().__init__()
        self.h = h
        self.encoder = torch.nn.Module()
        self.encoder.embeddings = table
        self.mean_count, self.local_step, self.iter_density, self.cuda_ray, self.bg_radius = 20000, 1, 16, True, 0
        self.register_buffer('step_counter', torch.zeros(16, 2, dtype=torch.int32))
        self.aabb_train = torch.zeros(6)
        self.w = torch.nn.Parameter(torch.zeros(()))

    def _fused_render_ok(self, rays_o, rays_d, bg, force_all_rays):
        return True

    def render(self, rays_o, rays_d, **kw):
        self.h.op('render')
        return {'image': (rays_o * 0 + self.w)}

    def refresh_occupancy(self, full):
        self.h.op(f'refresh(full={full})')
        return torch.zeros(())

    def refresh_sample(self, full):
        self.h.op(f'refresh_sample(full={full})')
        return torch.zeros(1)

    def refresh_apply(self, samples):
        self.h.op('refresh_apply')
        return torch.zeros(())

    def finish_update(self, mean, mean_count=None):
        self.h.log.append(f'finish_update(mean_count={mean_count})')
        self.iter_density += 1


def _install(monkeypatch, h, st_ref):
    import cmdlist
    import fused
    import optim

    @contextlib.contextmanager
    def graph(g, pool=None, capture_error_mode=None):
        if pool is None:
            h.n_pools += 1
            pool = f'own{h.n_pools}'
        g._pool, g.cap, h.capturing = pool, st_ref[0].captured_capacity, g
        try:
            yield
        finally:
            h.capturing = None
        h.log.append(f'capture({g.name},pool={pool})')

    @contextlib.contextmanager
    def stream(s):
        h.streams.append(s)
        try:
            yield
        finally:
            h.streams.pop()

    def new_pool():
        h.n_pools += 1
        return f'handle{h.n_pools}'

    def new_stream(device=None):
        h.n_streams += 1
        return _Stream(h, 'side' if h.n_streams == 1 else f'side{h.n_streams}')

    class Event:
        def __init__(self):
            self.name = (['la0', 'la1', 'sample', 'slot'] + [f'event{i}' for i in range(4, 64)])[h.n_events]
            h.n_events += 1

        def record(self, s=None):
            h.log.append(f'record({self.name},{(s or h.streams[-1]).name})')

    def which_set(target):
        la = getattr(st_ref[0], 'la_target', None) or ()
        return {id(t): str(p) for p, t in enumerate(la)}.get(id(target), '')

    def iteration(model, rays_o, rays_d, target, *a, noise_seed=None, found_inf=None, overwrite_table=None, table_adam=None, geo_loss=None):
        h.op('iteration' + ('[checked]' if found_inf is not None else '') + ('[table_adam]' if table_adam is not None else '')
             + ('[overwrite]' if overwrite_table else ''))
        return torch.full((1,), 7.0), torch.full((N, 3), 17.0), None

    def split(model, rays_o, rays_d, target, *a, noise_seed=None, found_inf=None, overwrite_table=None, table_adam=None, geo_loss=None):
        p = which_set(target)
        tags = ('[checked]' if found_inf is not None else '') + ('[table_adam]' if table_adam is not None else '') + ('[overwrite]' if overwrite_table else '')
        k = float(p or 0)

        def march():
            h.op(f'march{p}')

        def rest():
            h.op(f'rest{p}{tags}')
            return torch.full((1,), 10.0 + k), torch.full((N, 3), 20.0 + k)
        return march, rest

    for name, fn in dict(CUDAGraph=lambda: _Graph(h), graph=graph, graph_pool_handle=new_pool, Stream=new_stream, Event=Event,
                         current_stream=lambda *a, **k: h.streams[-1], stream=stream, synchronize=lambda *a, **k: None,
                         is_available=lambda: False).items():   # (the same log on a machine that has a GPU: nothing here may touch it)
        monkeypatch.setattr(torch.cuda, name, fn)
    monkeypatch.setattr(fused, 'fused_train_iteration', iteration)
    monkeypatch.setattr(fused, 'fused_train_iteration_split', split)
    monkeypatch.setattr(fused, 'iteration_checks_gradients', lambda model: True)
    monkeypatch.setattr(cmdlist, 'CommandList', lambda: _List(h))
    monkeypatch.setattr(optim, 'replayed_kept_deposits', lambda params: h.log.append(f'replayed_kept_deposits({len(params)})'))
    monkeypatch.setattr(optim, 'replayed_fused_table_step', lambda opt: h.log.append('replayed_fused_table_step'))


def _batch(k):
    return torch.full((1, N, 3), float(k)), torch.full((1, N, 3), k + 0.25), torch.full((N, 3), k + 0.5)


def _holds(o, d, t):
    """which batch a static buffer set holds: 'b3', or the three parts where they disagree"""
    ko, kd, kt = float(o.flatten()[0]), float(d.flatten()[0]) - 0.25, float(t.flatten()[0]) - 0.5
    assert bool((o == o.flatten()[0]).all() and (d == d.flatten()[0]).all() and (t == t.flatten()[0]).all())
    return f'b{ko:g}' if ko == kd == kt else f'o{ko:g}/d{kd:g}/t{kt:g}'


def _state(st, loss):
    s = [f'loss={float(loss):g}', f'image={float(st.image.flatten()[0]):g}', 'static=' + _holds(st.rays_o, st.rays_d, st.target)]
    if st.lookahead:
        s += ['la=' + ','.join(_holds(st.la_rays_o[p], st.la_rays_d[p], st.la_target[p]) for p in range(2)), f'seed={st.la_seed.tolist()}',
              f'la_cur={st.la_cur}', 'ready=' + ''.join('-' if r is None else 'x' for r in st.la_ready)]
    ring = st.model.step_counter[:, 0].tolist()
    s.append('ring=' + ','.join(f'{i}:{v}' for i, v in enumerate(ring) if v))
    s.append(f'steps={st.global_step}/{st.model.local_step}')
    return 'state ' + ' '.join(s)


def _figures(st):
    out = {k: getattr(st, k) for k in ('la_hits', 'la_presample_hits', 'n_switches', 'n_captures', 'n_list_replays', 'captures', 'capture_error',
                                       'update_capture_error', 'used_direct', 'table_fused', 'producers_check', '_checked_ok', 'capacity',
                                       'captured_capacity')}
    out['captured'] = sorted(st._captured)
    out['sharded'] = bool(getattr(st, 'sharded', False))
    out['has_la'] = getattr(st, 'la', None) is not None
    out['has_la_apply'] = getattr(st, 'la_apply', None) is not None
    out['has_lists'] = st.lists is not None
    out['n_graphs'] = None if st.graphs is None else len(st.graphs)
    out['update_graphs'] = sorted(st.update_graphs)
    out['ladder_error'] = getattr(st, 'ladder_error', None)
    return out


class _Run:
    def __init__(self, monkeypatch, first_step=1, shard=False, averager=False, table_fusion=False, march_at=None, **kw):
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'torch-ngp_amd'))
        from graph import GraphedTrainStep
        monkeypatch.setenv('NGP_STEP_CMDLIST', '1')
        monkeypatch.delenv('NGP_GRAPH_COLLECTIVES', raising=False)
        if march_at is None:
            monkeypatch.delenv('NGP_STEP_MARCH_AT', raising=False)
        else:
            monkeypatch.setenv('NGP_STEP_MARCH_AT', march_at)
        self.h = h = _Harness()
        ref = [None]
        _install(monkeypatch, h, ref)
        monkeypatch.setattr(GraphedTrainStep, '_table_fusion_fits', lambda self, emb: True)
        table = torch.nn.Parameter(torch.zeros(16, 2))
        table._ngp_fp16 = torch.zeros(16, 2, dtype=torch.half)
        opt = _Opt(h, [table, torch.nn.Parameter(torch.zeros(4))], shard=shard, table_fusion=table_fusion)
        kw.setdefault('capacity_ladder', ())
        self.st = st = GraphedTrainStep(_Model(h, table), opt, None, N, dict(perturb=True), averager=opt if averager else None,
                                        fused_table_adam=table_fusion, **kw)
        ref[0] = st
        st.global_step = first_step
        st.counter[:2, 0] = torch.tensor([100, 101], dtype=torch.int32)
        self.out = {'steps': []}

    def precapture(self):
        n = self.st.precapture()
        self.out['precapture'] = self.h.take() + [f'-> {n}']

    def step(self, batch, nxt=None):
        loss = self.st.step(*batch, **({} if nxt is None else dict(next_rays=nxt)))
        self.out['steps'].append(self.h.take() + [_state(self.st, loss)])

    def finish(self):
        self.out['figures'] = _figures(self.st)
        self.st.close()
        self.out['close'] = self.h.take()
        return self.out


def _plain(mp):
    r = _Run(mp, first_step=14, direct=False)
    r.precapture()
    for k in range(3):          # steps 14, 15 and 16: the last one begins with the refresh, replayed from its one graph
        r.step(_batch(k + 1))
    return r.finish()


def _plain_list(mp):
    r = _Run(mp, table_fusion=True)
    for k in range(2):
        r.step(_batch(k + 1))
    return r.finish()


def _replicated(mp):
    r = _Run(mp, averager=True)
    for k in range(2):
        r.step(_batch(k + 1))
    return r.finish()


def _sharded(mp):
    r = _Run(mp, averager=True, shard=True)
    b = [_batch(k) for k in range(6)]
    r.step(b[1])                       # nothing announced
    r.step(b[2], nxt=b[3])             # the next batch is copied behind the reduce-scatter ...
    r.step(b[3], nxt=b[4])             # ... and recognised: no copy in front of the march
    b[4][0].add_(0)                    # the announced tensor was written since: not the announced batch any more
    r.step(b[4], nxt=b[5])
    r.step(_batch(5))                  # equal values in other tensors: not the announced batch
    r.step(b[1], nxt=b[2][:2])         # rays without a target are not pre-copied
    return r.finish()


def _lookahead(mp):
    r = _Run(mp, first_step=11, lookahead=True, table_fusion=True)
    r.precapture()
    b = [_batch(k) for k in range(10)]
    r.step(b[1], nxt=b[2])             # 11: a miss (nothing was announced); marches b2 ahead, target announced
    r.step(b[2], nxt=b[3][:2])         # 12: a hit, target announced; b3 announced without its target
    r.step(b[3], nxt=b[4])             # 13: a hit, the target is copied now
    r.step(b[5], nxt=b[6])             # 14: another batch than the announced one: a miss behind the side stream's event
    r.step(b[6], nxt=b[7])             # 15: a hit; the step before a refresh does not look ahead: the refresh's cell sampling runs instead
    r.step(b[7], nxt=b[8])             # 16: the refresh (sampling already done), then a miss
    r.step(b[8], nxt=b[9])             # 17: a hit again
    return r.finish()


def _lookahead_refresh_first(mp):
    r = _Run(mp, first_step=16, lookahead=True)
    r.precapture()
    r.step(_batch(1))                  # the refresh's sampling half was not run ahead: both halves in line; nothing announced
    return r.finish()


def _marked_list(mp):
    r = _Run(mp, lookahead=True, table_fusion=True, march_at='net')
    b = [_batch(k) for k in range(5)]
    for k in range(1, 4):
        r.step(b[k], nxt=b[k + 1])
    return r.finish()


def _sharded_lookahead(mp, graphed=False):
    r = _Run(mp, averager=True, shard=True, lookahead=True)
    r.st.graph_collectives = graphed
    b = [_batch(k) for k in range(5)]
    for k in range(1, 4):
        r.step(b[k], nxt=b[k + 1])
    return r.finish()


def _switch(mp):
    r = _Run(mp, lookahead=True, capacity_ladder=(2.0,))
    r.precapture()
    b = [_batch(k) for k in range(6)]
    r.step(b[1], nxt=b[2])
    r.st.model.mean_count = 45000      # the estimate leaves the active buffer: the ladder's rung serves it, the marched-ahead batch is forgotten
    r.step(b[2], nxt=b[3])
    r.step(b[3], nxt=b[4])
    r.st.model.mean_count = 20000      # and back
    r.step(b[4], nxt=b[5])
    return r.finish()


def _capture_raises(mp):
    r = _Run(mp, direct=False)
    r.h.fail_graph_at = 0
    for k in range(2):
        r.step(_batch(k + 1))
    return r.finish()


def _precapture_raises(mp):
    r = _Run(mp, direct=False)
    r.h.fail_graph_at = 0
    r.precapture()
    r.step(_batch(1))
    return r.finish()


def _ladder_rung_raises(mp):
    r = _Run(mp, direct=False, capacity_ladder=(2.0,))
    r.h.fail_graph_at = 1              # the base capacity is captured, the rung is not: the base stays active
    r.precapture()
    r.step(_batch(1))
    return r.finish()


SCENARIOS = dict(plain=_plain, plain_list=_plain_list, replicated=_replicated, sharded=_sharded, lookahead=_lookahead,
                 lookahead_refresh_first=_lookahead_refresh_first, marked_list=_marked_list, sharded_lookahead_apply=_sharded_lookahead,
                 sharded_lookahead_graph_collectives=lambda mp: _sharded_lookahead(mp, graphed=True), switch=_switch,
                 capture_raises=_capture_raises, precapture_raises=_precapture_raises, ladder_rung_raises=_ladder_rung_raises)


@pytest.mark.filterwarnings('ignore:.*CUDA is not available.*')
@pytest.mark.parametrize('scenario', sorted(SCENARIOS))
def test_step_issues_what_the_golden_log_holds(monkeypatch, scenario):
    with open(GOLDEN) as f:
        want = json.load(f)[scenario]
    got = json.loads(json.dumps(SCENARIOS[scenario](monkeypatch)))
    assert sorted(got) == sorted(want)
    for i, (g, w) in enumerate(zip(got['steps'], want['steps'])):
        assert g == w, f'{scenario}: step {i}'
    for part in want:
        assert got[part] == want[part], f'{scenario}: {part}'


def test_the_golden_log_covers_every_path():
    """the golden file itself: every scenario is present and went down the path it is named after"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(SCENARIOS)
    la = gold['sharded_lookahead_apply']
    assert la['figures']['la_hits'] == 2 and la['figures']['has_la_apply']
    flat = [e for s in gold['switch']['steps'] for e in s]
    assert gold['switch']['figures']['n_switches'] >= 2 and any('@49152' in e for e in flat)
    assert gold['capture_raises']['figures']['capture_error'] is not None
    assert any('captures_discarded' in e for e in gold['capture_raises']['steps'][0])
