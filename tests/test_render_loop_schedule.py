"""CPU checks of the eval render loop's host policy (nerf/render_loop.py: LoopOptions, Schedule) -- no GPU, no native library:
- parity with the parent: the read-backs recorded in tests/golden/render_loop_schedule.json (tools/render_loop_schedule_dump.py, run on the
  commit the file names, before the module existed) replayed through Schedule give the recorded `_loop_debug` tuples for the native pair
  call and for the per-stage loop, and the recorded per-iteration (lanes, rows, n_total) for the per-stage loop.  The golden holds no
  per-iteration data of the native mode (the stage probe that records them declines the native call): its rows and lanes, which follow
  `device_rows` and its batch growth, are pinned against the parent only through the `done` column of `_loop_debug`, and against the
  kernels' bound by the second group of tests;
- the bound the kernels rely on: k_march_rays writes n_alive * n_step rows unchecked and the composite / compaction kernels trust `lanes`,
  so every batch must hold every alive count the device may reach before the next read-back;
- the precedence of the knobs."""
import itertools
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

from nerf.render_loop import LoopOptions, Schedule

MAX_STEPS = 1024


@pytest.fixture(autouse=True)
def _no_loop_environment(monkeypatch):
    monkeypatch.delenv('NGP_LOOP_INITIAL_BOOST', raising=False)
    monkeypatch.delenv('NGP_LOOP_TAIL_CAP', raising=False)


def pad(rows):
    """the marchers' padding rule (raymarching._round_up_strict(rows, 128), restated: that module loads the native library)"""
    return rows + 128 - rows % 128


def n_step(n_total, n_alive, cap):
    """loop_n_step of csrc/raymarching.hip, on an array of alive counts"""
    if cap == 0:
        cap = 8
    q = n_total // np.maximum(n_alive, 1)
    return np.where(n_alive == 0, 1, np.where(q > cap, cap, np.where(q < 1, 1, q)))


def options(*args, **kwargs):
    """every knob read, as FrameLoop has them once the frame is seeded"""
    return LoopOptions(*args, **kwargs).read_policy()


def stub(**attrs):
    """what LoopOptions reads of a model when no knob is set"""
    return SimpleNamespace(grid_size=128, forward_scaled=None, **attrs)


# ---- parity with the parent ---------------------------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'render_loop_schedule.json')) as f:
        return json.load(f)


def _replay(frame, mode):
    """the frame's recorded read-backs through a Schedule -> (the _loop_debug tuples, (lanes, rows, n_total) per iteration)"""
    rec = frame[mode]
    opt = options(stub(native_loop=mode == 'native', _loop_probe=None if mode == 'native' else []), perturb=frame['perturb'])
    assert opt.native == (mode == 'native')
    schedule = Schedule(frame['n_rays'], MAX_STEPS, opt, pad)
    device_rows = rec['device_rows']
    batch = schedule.first()
    debug, iterations = [], [[batch.lanes, batch.rows, batch.n_total]] * 2
    for alive in [d[1] for d in rec['debug']] + [rec['final_alive']]:
        batch = schedule.next(alive, device_rows)
        if batch is None:
            break
        debug.append(list(batch.debug))
        iterations += [[batch.lanes, batch.rows, batch.n_total]] * (2 * batch.pairs)
    assert schedule.next(rec['final_alive'], device_rows) is None, 'the parent stopped here'
    return debug, iterations


def test_schedule_reproduces_the_parents_frames():
    golden = _golden()
    assert len(golden['frames']) == 6
    for frame in golden['frames']:
        for mode in ('native', 'stages'):
            debug, iterations = _replay(frame, mode)
            where = (frame['n_rays'], frame['density_scale'], mode)
            assert debug == frame[mode]['debug'], where
            if mode == 'stages':
                assert iterations == [it[:3] for it in frame[mode]['iterations']], where


def test_parents_recorded_alive_counts_fit_their_launches():
    """(what the device really held, iteration by iteration, against what the host had sized)"""
    for frame in _golden()['frames']:
        its = np.array(frame['stages']['iterations'])
        lanes, rows, n_total, alive = its.T
        assert (alive <= lanes).all() and (rows % 128 == 0).all()
        assert (alive * n_step(n_total, alive, 8) <= rows).all()   # (cap <= what was issued: fewer rows than the true cap gives would fail too)


# ---- the bound the kernels rely on --------------------------------------------------------------------------------------------------------
def _check_batch(batch, n_rays, bound_alive, tail_cap, graphs):
    assert batch.rows > 0 and batch.rows % 128 == 0
    assert batch.lanes >= bound_alive
    if n_rays <= 4096:
        a = np.arange(1, bound_alive + 1)
    else:
        picks = {bound_alive, bound_alive // 2, 1}
        for c in {8, batch.cap}:
            if c:
                picks |= {batch.n_total // c, batch.n_total // c + 1}
        a = np.array(sorted(p for p in picks if 1 <= p <= bound_alive))
    worst = a * n_step(batch.n_total, a, batch.cap)
    assert worst.max() <= batch.rows, (batch, int(a[worst.argmax()]))
    if graphs:
        k = (batch.n_total // batch.bucket).bit_length() - 1
        assert batch.bucket == batch.n_total >> k and (batch.bucket >= 2048 or batch.bucket == batch.n_total), batch


@pytest.mark.parametrize('n_rays', [1, 7, 100, 2047, 2048, 4096, 20000, 640000])
def test_every_batch_holds_every_alive_count_until_the_next_read_back(n_rays):
    runs = 0
    for graphs, perturb, device_rows, tail_cap, survival in itertools.product(
            (False, True), (False, True), (False, True), (8, 64, 1024), (0.999, 0.97, 0.9, 0.7, 0.3, 0.05)):
        opt = options(stub(graph_loop=graphs, loop_tail_cap=tail_cap), perturb=perturb)
        assert opt.graphs == graphs and opt.tail_cap == (8 if graphs else tail_cap)
        schedule = Schedule(n_rays, MAX_STEPS, opt, pad)
        rng = random.Random(n_rays * 1000 + runs)
        batch = schedule.first()
        assert (batch.lanes, batch.n_total, batch.cap) == (n_rays, opt.initial_boost * n_rays, 0)
        _check_batch(batch, n_rays, n_rays, tail_cap, False)
        alive, iters, done = n_rays, 2, 2
        while True:
            for _ in range(iters):   # non-increasing: the per-iteration survival, jittered downwards
                alive = min(alive, int(alive * survival * rng.uniform(0.97, 1.0) + rng.random()))
            batch = schedule.next(alive, device_rows)
            if batch is None:
                break
            _check_batch(batch, n_rays, alive, tail_cap, graphs)
            iters = 2 * batch.pairs
            done += iters
            assert schedule.done == done and 1 <= batch.pairs <= 4
        assert alive == 0 or done >= MAX_STEPS
        runs += 1
    assert runs == 144


def test_a_failed_capture_only_switches_the_rest_of_the_frame_to_eager_issue():
    opt = options(stub(graph_loop=True))
    a, b = Schedule(20000, MAX_STEPS, opt, pad), Schedule(20000, MAX_STEPS, opt, pad)
    assert a.first() == b.first() and a.next(9000, False) == b.next(9000, False)
    b.capture_failed()
    assert a.graphs and not b.graphs
    ga, gb = a.next(700, False), b.next(700, False)
    assert (gb.lanes, gb.rows) == (700, pad(8 * 700)) and (ga.lanes, ga.rows) == (ga.bucket // 8 + 1, pad(ga.bucket))
    assert ga._replace(lanes=0, rows=0) == gb._replace(lanes=0, rows=0)   # still the fixed n_step rule: adaptive off, cap 8


def test_the_tail_rule_waits_for_the_second_read_back():
    """a frame whose FIRST read-back is already in the tail (alive * 16 <= N): the parent applies the tail's batch size behind the read-backs
    inside its loop only, so the first batch is one pair whatever `device_rows` says.  By hand, N = 4096, first read-back 100 rays:
    cap = clamp(4096 // 100, 8, 64) = 40, survival (100 / 4096) ** (1 / 2) < 0.75 at boost 1, need = 40 * 100 = 4000 -> rows 4096;
    second read-back 10 rays: cap 64, need 640 -> rows 768, and now the tail's batch: two pairs with device-side row counts, one without"""
    for device_rows in (True, False):
        schedule = Schedule(4096, MAX_STEPS, options(stub()), pad)
        schedule.first()
        assert schedule.next(100, device_rows) == (1, 100, 4096, 4096, 40, 4096, (2, 100, 1, 0.156))
        assert schedule.next(10, device_rows) == (2 if device_rows else 1, 10, 768, 4096, 64, 2048, (4, 10, 1, 0.316))
        assert schedule.done == (8 if device_rows else 6)


# ---- option precedence --------------------------------------------------------------------------------------------------------------------
def test_environment_against_attributes(monkeypatch):
    opt = options(stub())
    assert (opt.initial_boost, opt.tail_cap, opt.max_rows, opt.sync_every) == (2, 64, 1 << 26, 8)
    assert options(stub(loop_initial_boost=3, loop_tail_cap=32)).initial_boost == 3
    monkeypatch.setenv('NGP_LOOP_INITIAL_BOOST', '4')
    monkeypatch.setenv('NGP_LOOP_TAIL_CAP', '16')
    opt = options(stub())
    assert (opt.initial_boost, opt.tail_cap) == (4, 16)
    opt = options(stub(loop_initial_boost=3, loop_tail_cap=32))
    assert (opt.initial_boost, opt.tail_cap) == (4, 32), 'the environment wins for the boost, the attribute for the tail cap'
    assert options(stub(loop_initial_boost=3), perturb=True).initial_boost == 1
    assert options(stub(loop_tail_cap=4)).tail_cap == 8 and options(stub(loop_tail_cap=5000)).tail_cap == 1024
    monkeypatch.setenv('NGP_LOOP_INITIAL_BOOST', '0')
    assert options(stub()).initial_boost == 1


def test_what_declines_graphs_the_native_call_the_adaptive_policy_and_culling():
    aux = lambda *a: None   # noqa: E731
    opt = options(stub())
    assert (opt.graphs, opt.adaptive, opt.native, opt.cull, opt.device_rows) == (False, True, True, True, True)
    opt = options(stub(graph_loop=True, loop_tail_cap=64))
    assert (opt.graphs, opt.adaptive, opt.tail_cap, opt.native) == (True, False, 8, True)
    opt = options(stub(graph_loop=True), graphs_failed=True)
    assert (opt.graphs, opt.adaptive, opt.tail_cap) == (False, True, 64)
    opt = options(stub(graph_loop=True), aux_infer=aux)
    assert (opt.graphs, opt.native, opt.adaptive, opt.cull, opt.tail_cap) == (False, False, True, True, 64)
    assert options(stub(adaptive_n_step=False)).tail_cap == 8
    for declined in (dict(native_loop=False), dict(_loop_probe=[]), dict(_loop_iter_hook=print)):
        assert not options(stub(**declined)).native, declined
    assert not options(SimpleNamespace(grid_size=128)).native, 'no forward_scaled on the model'
    assert not options(stub(loop_device_rows=False)).device_rows
    assert not options(stub(), perturb=True).cull and not options(stub(cull_empty_rays=False)).cull
    for grid_size, cull in ((8, False), (16, True), (96, False), (128, True)):
        assert options(SimpleNamespace(grid_size=grid_size)).cull == cull, grid_size
