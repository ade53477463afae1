"""GPU checks of the inference loop's kernels at the C ABI (include/ngp_hip.h): ngp_composite_rays / ngp_composite_rays_dev (k_composite_rays),
ngp_compact_rays / ngp_compact_rays_dev (k_compact_count, k_compact_write), ngp_march_rays_dev / ngp_march_rays_dev_rows against
ngp_march_rays_ex (k_march_rays), and the whole loop on device-side state without a host read-back -- on the cases of
tests/render_loop_cases.py, against its float64 definition (tests/test_render_loop_cases.py pins that definition to the oracle and, where
built, to the reference's own kernel).

Tolerance of every floating output: 4 x (error of the float32 model of the same statements against the float64 definition, same inputs) +
1e-7 x (largest reference magnitude); alive lists, compaction results, loop state, rows_used and every "unchanged" claim are exact.

Measured on MI355X, kernel error / bound per output (the float32 model's exponential is numpy's fp32 exp; the kernel's __expf stayed well
inside, so the exp2 restatement render_loop_cases offers was not needed):
    n_step            weights_sum   depth   image   rays_t
    1                    0.073      0.124   0.130   0.155
    2                    0.139      0.183   0.180   0.168
    3                    0.084      0.130   0.179   0.192
    8                    0.101      0.101   0.191   0.219
    13                   0.085      0.222   0.151   0.217
    64                   0.137      0.233   0.208   0.226
    3 calls of 4         0.182      0.162   0.273   0.208
    whole loop           0.170      0.206   0.213     --      (the 1437 of 2000 rays that stay off T_thresh; bounds 2.1e-6 / 1.7e-5 / 5.4e-6)
(rays_t: the kernel's error EQUALS the float32 model's in every table -- the same fp32 additions.)  The 563 rays of the whole loop that come
within the weights_sum bound of T_thresh are at most 6.8e-6 / 2.2e-5 / 7.1e-6 off (weights_sum / depth / image), against the extra
T_thresh x (1, largest t, largest rgb) = 1e-4 / 4.8e-4 / 1e-4 they are granted.  Every test prints its figures before it asserts
(pytest -s).  The whole file takes about 7 s, 3 s of it the whole loop (most of that the float64 / float32 model loops on the CPU).
"""
import functools

import numpy as np
import pytest
import torch

import oracle
import render_loop_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 123.25
MARCH = dict(bound=1.0, dt_gamma=0.0, max_steps=1024, C=1, H=128)


def _capi():
    import _ngp_capi as capi
    return capi


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# ngp_composite_rays
# ------------------------------------------------------------------------------------------------
def _upload(call, rays_alive=None, rows=None):
    """one call's tensors on the device; `rows` > n_alive * n_step: the sample buffers are that long, the extra rows hold ordinary-looking
    (non-zero) samples that nothing may read"""
    n = call['n_alive'] * call['n_step']
    sg, rg, de = call['sigmas'].reshape(-1), call['rgbs'].reshape(-1, 3), call['deltas'].reshape(-1, 2)
    if rows is not None and rows > n:
        a, b, c = C._rows(np.random.default_rng(5), rows - n, 1)
        sg, rg, de = np.concatenate([sg, a.reshape(-1)]), np.concatenate([rg, b.reshape(-1, 3)]), np.concatenate([de, c.reshape(-1, 2)])
    s = {k: cu(call[k].astype(np.float32)) for k in C.KEYS}
    s.update(rays_alive=cu(call['rays_alive'] if rays_alive is None else rays_alive), sigmas=cu(sg), rgbs=cu(rg), deltas=cu(de))
    return s


def _clone(s):
    return {k: v.clone() for k, v in s.items()}


def _composite(s, n_alive, n_step, T_thresh):
    capi = _capi()
    capi.check(capi.lib.ngp_composite_rays(n_alive, n_step, T_thresh, p(s['rays_alive']), p(s['rays_t']), p(s['sigmas']), p(s['rgbs']), p(s['deltas']),
                                           p(s['weights_sum']), p(s['depth']), p(s['image']), capi.stream()))
    torch.cuda.synchronize()


def _composite_dev(s, state, alive_bound, n_total, cap, T_thresh):
    capi = _capi()
    capi.check(capi.lib.ngp_composite_rays_dev(p(state), alive_bound, n_total, cap, T_thresh, p(s['rays_alive']), p(s['rays_t']), p(s['sigmas']),
                                               p(s['rgbs']), p(s['deltas']), p(s['weights_sum']), p(s['depth']), p(s['image']), capi.stream()))
    torch.cuda.synchronize()


def _check_values(got, ref, bounds, what):
    for key in C.KEYS:
        err = float(np.abs(got[key].double().cpu().numpy() - ref[key]).max())
        bound = bounds[key][0]
        print(f'{what} {key}: kernel error {err:.3e}, float32 model error {bounds[key][1]:.3e}, bound {bound:.3e}, err / bound {err / bound:.3f}')
        assert err <= bound, (what, key, err, bound)


@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_composite_rays_matches_the_float64_definition(n_step):
    t, ref, bounds = C.composite_table(n_step), C.table_reference(n_step), C.yardstick(n_step)
    s = _upload(t)
    before = _clone(s)
    _composite(s, t['n_alive'], n_step, t['T_thresh'])
    _check_values(s, ref, bounds, f'composite_rays n_step={n_step}')
    assert np.array_equal(s['rays_alive'].cpu().numpy(), ref['rays_alive'])           # exactly: no ray of the table is near T_thresh
    stopped = cu(t['rays_alive'][ref['rays_alive'] < 0].astype(np.int64))
    assert len(stopped) >= 5 and _same_bits(s['rays_t'][stopped], before['rays_t'][stopped])
    moved = cu(t['rays_alive'][ref['rays_alive'] >= 0].astype(np.int64))
    assert (s['rays_t'][moved] != before['rays_t'][moved]).all()
    outside = cu(t['outside'].astype(np.int64))
    for key in C.KEYS:   # the 36 rays that are not in the list
        assert _same_bits(s[key][outside], before[key][outside]), key
    for key in ('sigmas', 'rgbs', 'deltas'):
        assert _same_bits(s[key], before[key])


def test_composite_rays_three_consecutive_calls():
    calls = C.multi_call_table()
    ref, lists, bounds = C.multi_yardstick()
    s = _upload(calls[0])
    for i, call in enumerate(calls):
        assert np.array_equal(s['rays_alive'].cpu().numpy(), call['rays_alive'])   # the compacted list of the kernel's own previous call
        s.update(sigmas=cu(call['sigmas'].reshape(-1)), rgbs=cu(call['rgbs'].reshape(-1, 3)), deltas=cu(call['deltas'].reshape(-1, 2)))
        _composite(s, call['n_alive'], call['n_step'], call['T_thresh'])
        assert np.array_equal(s['rays_alive'].cpu().numpy(), lists[i]), i
        s['rays_alive'] = s['rays_alive'][s['rays_alive'] >= 0].contiguous()
    _check_values(s, ref, bounds, 'composite_rays, 3 calls of n_step=4')


def test_composite_rays_two_calls_give_the_same_bits():
    t = C.composite_table(8)
    a, b = _upload(t), _upload(t)
    _composite(a, t['n_alive'], 8, t['T_thresh'])
    _composite(b, t['n_alive'], 8, t['T_thresh'])
    for key in a:
        assert _same_bits(a[key], b[key]) and not torch.isnan(a[key].float()).any(), key


def test_composite_rays_with_an_empty_list_writes_nothing():
    t = C.composite_table(3)
    s = _upload(t)
    before = _clone(s)
    _composite(s, 0, 3, t['T_thresh'])
    for key in s:
        assert _same_bits(s[key], before[key]), key


# ------------------------------------------------------------------------------------------------
# ngp_composite_rays_dev
# ------------------------------------------------------------------------------------------------
# (n_total, cap) from which the device derives each n_step of the table for the 61 rays of the list
DEV_N_STEP = {1: (61, 0), 2: (4096, 2), 3: (200, 0), 8: (4096, 0), 13: (4096, 13), 64: (4096, 64)}


@pytest.mark.parametrize('alive_bound', [61, 64, 300])
@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_composite_rays_dev_equals_the_host_entry(n_step, alive_bound):
    t = C.composite_table(n_step)
    n_total, cap = DEV_N_STEP[n_step]
    assert C.loop_n_step(n_total, 61, cap) == n_step
    # list entries [61, alive_bound): valid ids of rays OUTSIDE the list; sample rows behind the 61 rays': ordinary non-zero samples
    full_list = np.concatenate([t['rays_alive'], np.resize(t['outside'], alive_bound - 61)]).astype(np.int32)
    host = _upload(t, full_list, rows=alive_bound * n_step)
    dev = _clone(host)
    before = _clone(host)
    _composite(host, 61, n_step, t['T_thresh'])
    state = cu(np.array([61, 17], np.int32))
    _composite_dev(dev, state, alive_bound, n_total, cap, t['T_thresh'])
    for key in host:
        assert _same_bits(host[key], dev[key]), key
    assert state.cpu().tolist() == [61, 17]
    assert (dev['rays_alive'][:61] < 0).any() and _same_bits(dev['rays_alive'][61:], before['rays_alive'][61:])
    outside = cu(t['outside'].astype(np.int64))
    for key in C.KEYS:
        assert _same_bits(dev[key][outside], before[key][outside]), key
    listed = cu(t['rays_alive'].astype(np.int64))
    assert not _same_bits(dev['weights_sum'][listed], before['weights_sum'][listed])


@pytest.mark.parametrize('cap', [0, 64])
def test_composite_rays_dev_with_a_device_count_of_zero_changes_nothing(cap):
    t = C.composite_table(8)
    full_list = np.concatenate([t['rays_alive'], np.resize(t['outside'], 300 - 61)]).astype(np.int32)
    s = _upload(t, full_list, rows=300 * 8)
    before = _clone(s)
    state = cu(np.array([0, 17], np.int32))
    _composite_dev(s, state, 300, 4096, cap, t['T_thresh'])
    for key in s:
        assert _same_bits(s[key], before[key]), key
    assert state.cpu().tolist() == [0, 17]


# ------------------------------------------------------------------------------------------------
# ngp_compact_rays / ngp_compact_rays_dev
# ------------------------------------------------------------------------------------------------
GUARD = 64


def _workspace(nbytes):
    """exactly `nbytes` of workspace, followed by guard bytes that must survive"""
    big = torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device='cuda')
    return big, big[:nbytes]


def _compact(a_dev, n):
    capi = _capi()
    out = torch.full((a_dev.shape[0],), C.FILL, dtype=torch.int32, device='cuda')
    cnt = torch.full((1,), -3, dtype=torch.int32, device='cuda')
    nbytes = int(capi.lib.ngp_compact_rays_workspace_bytes(n))
    assert nbytes == 4 * max(1, -(-n // 256))
    big, ws = _workspace(nbytes)
    capi.check(capi.lib.ngp_compact_rays(p(a_dev), n, p(out), p(cnt), p(ws), capi.stream()))
    torch.cuda.synchronize()
    assert (big[nbytes:] == 0xAB).all()
    return out, int(cnt.item())


def _compact_dev(a_dev, state, alive_bound, n_total, cap, max_steps):
    capi = _capi()
    assert a_dev.shape[0] >= alive_bound
    out = torch.full((a_dev.shape[0],), C.FILL, dtype=torch.int32, device='cuda')
    out_state = torch.full((2,), -3, dtype=torch.int32, device='cuda')
    nbytes = int(capi.lib.ngp_compact_rays_workspace_bytes(alive_bound))
    big, ws = _workspace(nbytes)
    capi.check(capi.lib.ngp_compact_rays_dev(p(state), alive_bound, n_total, cap, max_steps, p(a_dev), p(out), p(out_state), p(ws), capi.stream()))
    torch.cuda.synchronize()
    assert (big[nbytes:] == 0xAB).all()
    return out, out_state.cpu().tolist()


@pytest.mark.parametrize('n', C.COMPACT_SIZES)
def test_compact_rays(n):
    for pattern in C.COMPACT_PATTERNS:
        a, want = C.compaction_case(n, pattern)
        a_dev = cu(a)
        out, count = _compact(a_dev, n)
        out = out.cpu().numpy()
        assert count == len(want), (pattern, count, len(want))
        assert np.array_equal(out[:count], want), pattern
        assert (out[n:] == C.FILL).all() and len(out) == n + C.TAIL, pattern     # nothing behind n_alive is read as a ray or written
        assert np.array_equal(a_dev.cpu().numpy(), a), pattern


@pytest.mark.parametrize('n', [n for n in C.COMPACT_SIZES if n <= 70001])
def test_compact_rays_dev(n):
    n_total, s0 = 4096, 5
    for k, pattern in enumerate(C.COMPACT_PATTERNS):
        a, want = C.compaction_case(n, pattern, length=2 * n + 7)
        a_dev = cu(a)
        host_out, host_count = _compact(a_dev, n)
        assert host_count == len(want)
        cap = (0, 64)[k % 2]
        n_step = C.loop_n_step(n_total, n, cap)
        for alive_bound in (n, n + 1, n + 255, 2 * n + 7):
            state = cu(np.array([n, s0], np.int32))
            out, out_state = _compact_dev(a_dev, state, alive_bound, n_total, cap, 10 ** 6)
            assert out_state == [len(want), s0 + n_step], (pattern, alive_bound, out_state)
            assert torch.equal(out[:host_count], host_out[:host_count]) and np.array_equal(out[:host_count].cpu().numpy(), want), (pattern, alive_bound)
            assert (out[n:] == C.FILL).all(), (pattern, alive_bound)
            assert state.cpu().tolist() == [n, s0]
        assert np.array_equal(a_dev.cpu().numpy(), a), pattern
    # the forced 0 once max_steps samples are marched: one step below the limit, exactly at it, above it
    a, want = C.compaction_case(n, 'all alive', length=2 * n + 7)
    a_dev = cu(a)
    for cap in (0, 64):
        done = s0 + C.loop_n_step(n_total, n, cap)
        for max_steps, cut in ((done + 1, False), (done, True), (done - 1, True)):
            out, out_state = _compact_dev(a_dev, cu(np.array([n, s0], np.int32)), n + 255, n_total, cap, max_steps)
            assert out_state == [0 if cut else n, done], (cap, max_steps, out_state)
            assert np.array_equal(out[:n].cpu().numpy(), want)       # the list itself is compacted either way


@pytest.mark.parametrize('alive_bound', [1, 300, 70001])
def test_compact_rays_dev_true_count_of_zero_under_a_positive_bound(alive_bound):
    a, _ = C.compaction_case(0, 'all alive', length=alive_bound)     # nothing but valid-looking ids
    a_dev = cu(a)
    for cap in (0, 64):
        out, out_state = _compact_dev(a_dev, cu(np.array([0, 9], np.int32)), alive_bound, 4096, cap, 10 ** 6)
        assert out_state == [0, 10] and (out == C.FILL).all()


# ------------------------------------------------------------------------------------------------
# ngp_march_rays_dev_rows / ngp_march_rays_dev against ngp_march_rays_ex
# ------------------------------------------------------------------------------------------------
MARCH_N = 600


@functools.lru_cache(maxsize=None)
def _march_scene():
    bits = C.scene(1.0, 1)
    o, d = C.random_rays(MARCH_N, 41)
    nears, fars = oracle.near_far_from_aabb(o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32), 0.2)
    rng = np.random.default_rng(42)
    rays_t = (nears + rng.uniform(0.0, 1.2, MARCH_N)).astype(np.float32)      # rays at different depths of the scene, some behind it
    perm = rng.permutation(MARCH_N).astype(np.int32)
    return dict(bits=cu(bits), o=cu(o), d=cu(d), nears=cu(nears), fars=cu(fars), rays_t=cu(rays_t), perm=perm)


def _sample_buffers(rows):
    return [torch.full((rows, k), SENTINEL, device='cuda') for k in (3, 3, 2)]


def _march_ex(sc, n, n_step, rays_alive, noises, zero_rows, alloc):
    capi = _capi()
    x, dd, de = _sample_buffers(alloc)
    m = MARCH
    capi.check(capi.lib.ngp_march_rays_ex(n, n_step, p(rays_alive), p(sc['rays_t']), p(sc['o']), p(sc['d']), m['bound'], m['dt_gamma'], m['max_steps'],
                                          m['C'], m['H'], p(sc['bits']), p(sc['nears']), p(sc['fars']), p(x), p(dd), p(de), p(noises), zero_rows,
                                          capi.stream()))
    torch.cuda.synchronize()
    return x, dd, de


def _march_dev(sc, state, alive_bound, n_total, cap, rays_alive, noises, rows, alloc, publish):
    capi = _capi()
    assert rays_alive.shape[0] >= alive_bound and alloc >= rows
    x, dd, de = _sample_buffers(alloc)
    m = MARCH
    args = (p(state), alive_bound, n_total, cap, p(rays_alive), p(sc['rays_t']), p(sc['o']), p(sc['d']), m['bound'], m['dt_gamma'], m['max_steps'],
            m['C'], m['H'], p(sc['bits']), p(sc['nears']), p(sc['fars']), p(x), p(dd), p(de), p(noises), rows)
    if publish:
        used = torch.full((1,), -3, dtype=torch.int32, device='cuda')
        capi.check(capi.lib.ngp_march_rays_dev_rows(*args, p(used), capi.stream()))
    else:
        used = None
        capi.check(capi.lib.ngp_march_rays_dev(*args, capi.stream()))
    torch.cuda.synchronize()
    return (x, dd, de), (None if used is None else int(used.item()))


@pytest.mark.parametrize('n_total,n,cap,n_step', [row for row in C.LADDER if row[1] > 0])
def test_march_rays_dev_rows(n_total, n, cap, n_step):
    """ladder rows -> n_step 1 (4096 and 5000 list entries: ray ids repeat, which the marcher, reading rays only, does not mind), 4, 8, 40, 64;
    n * n_step is a multiple of 128 for (4096, 4096), (4096, 512) and (4096, 10, 64): a full extra 128 rows"""
    sc = _march_scene()
    used = n * n_step
    aligned = used % 128 == 0
    assert aligned == ((n, cap) in ((4096, 0), (512, 0), (10, 64)))
    noises_real = cu(np.random.default_rng(n).random(n + 200, dtype=np.float32))
    for alive_bound in (n, n + 200):
        rays_alive = cu(np.resize(sc['perm'], alive_bound))
        state = cu(np.array([n, 3], np.int32))
        for rows in (used + 300, used + 1):       # the padded count is the smaller term / `rows` is
            alloc = rows + 64
            want_used = C.rows_used(rows, n, n_step)
            assert want_used == (min(rows, used + 128) if aligned else min(rows, -(-used // 128) * 128))
            for noises in (None, noises_real):
                got, got_used = _march_dev(sc, state, alive_bound, n_total, cap, rays_alive, noises, rows, alloc, publish=True)
                assert got_used == want_used, (alive_bound, rows, got_used, want_used)
                # NULL noises = no perturbation: the reference call gets explicit zeros
                ref_noises = torch.zeros(n, device='cuda') if noises is None else noises
                ref = _march_ex(sc, n, n_step, rays_alive, ref_noises, want_used, alloc)
                for g, r in zip(got, ref):
                    assert _same_bits(g[:want_used], r[:want_used])
                    assert (g[want_used:] == SENTINEL).all()             # rows [rows_used, rows) and the spare rows behind `rows`: untouched
                # rows_used == NULL (ngp_march_rays_dev): everything up to `rows` is zero-filled
                got0, _ = _march_dev(sc, state, alive_bound, n_total, cap, rays_alive, noises, rows, alloc, publish=False)
                ref0 = _march_ex(sc, n, n_step, rays_alive, ref_noises, rows, alloc)
                for g, r in zip(got0, ref0):
                    assert _same_bits(g, r) and not g[used:rows].any() and (g[rows:] == SENTINEL).all()
                emitted = got[2][:used, 0] > 0
                assert emitted.any() and (n < 100 or not emitted.all())    # samples and empty slots
        assert state.cpu().tolist() == [n, 3]


@pytest.mark.parametrize('n_total,n,cap,n_step', [row for row in C.LADDER if row[1] == 0])
def test_march_rays_dev_with_a_device_count_of_zero(n_total, n, cap, n_step):
    sc = _march_scene()
    rays_alive = cu(np.resize(sc['perm'], 300))
    state = cu(np.array([0, 3], np.int32))
    for rows in (1000, 128, 100):
        got, got_used = _march_dev(sc, state, 300, n_total, cap, rays_alive, None, rows, rows + 64, publish=True)
        assert got_used == min(rows, 128) == C.rows_used(rows, 0, n_step)
        for g in got:
            assert not g[:got_used].any() and (g[got_used:] == SENTINEL).all()      # all of it zero: no sample
        got0, _ = _march_dev(sc, state, 300, n_total, cap, rays_alive, None, rows, rows + 64, publish=False)
        for g in got0:
            assert not g[:rows].any() and (g[rows:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------
# the whole loop at the ABI
# ------------------------------------------------------------------------------------------------
def _fields_on_device(xyzs):
    """render_loop_cases.fields64 with torch ops on the device: float64, rounded once to fp32"""
    x = xyzs.double()
    sig = 25.0 * torch.exp(-3.0 * (x ** 2).sum(-1)) + 2.0 * (x[:, 0] > 0.2)
    rgb = 0.5 + 0.5 * torch.sin(3.0 * x + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=x.device))
    return sig.float().contiguous(), rgb.float().contiguous()


def _run_loop(cap, n_iter):
    """n_iter iterations march -> fields -> composite -> compact on ping-pong alive lists / states, alive_bound = N throughout, no read-back
    before the end -> (weights_sum, depth, image, rays_t, final state)"""
    capi = _capi()
    inp = C.loop_inputs()
    N, m = C.LOOP_N, MARCH
    rows = N + 128                                        # n_alive * n_step <= N for every count, + the padding
    o, d, bits, nears, fars = (cu(inp[k]) for k in ('o', 'd', 'bits', 'nears', 'fars'))
    alive = [torch.arange(N, dtype=torch.int32, device='cuda'), torch.zeros(N, dtype=torch.int32, device='cuda')]
    state = cu(np.array([[N, 0], [0, 0]], np.int32))
    rays_t = cu(inp['nears']).clone()
    ws, dep, img = torch.zeros(N, device='cuda'), torch.zeros(N, device='cuda'), torch.zeros(N, 3, device='cuda')
    xyzs, dirs, deltas = torch.zeros(rows, 3, device='cuda'), torch.zeros(rows, 3, device='cuda'), torch.zeros(rows, 2, device='cuda')
    used = torch.zeros(1, dtype=torch.int32, device='cuda')
    work = torch.empty(int(capi.lib.ngp_compact_rays_workspace_bytes(N)), dtype=torch.uint8, device='cuda')
    stream = capi.stream()
    for i in range(n_iter):
        cur = i & 1
        st, st_next = state.data_ptr() + 8 * cur, state.data_ptr() + 8 * (cur ^ 1)
        capi.check(capi.lib.ngp_march_rays_dev_rows(st, N, N, cap, p(alive[cur]), p(rays_t), p(o), p(d), m['bound'], m['dt_gamma'], m['max_steps'], m['C'],
                                                    m['H'], p(bits), p(nears), p(fars), p(xyzs), p(dirs), p(deltas), None, rows, p(used), stream))
        sig, rgb = _fields_on_device(xyzs)
        capi.check(capi.lib.ngp_composite_rays_dev(st, N, N, cap, C.LOOP_T_THRESH, p(alive[cur]), p(rays_t), p(sig), p(rgb), p(deltas), p(ws), p(dep),
                                                   p(img), stream))
        capi.check(capi.lib.ngp_compact_rays_dev(st, N, N, cap, C.LOOP_MAX_STEPS, p(alive[cur]), p(alive[cur ^ 1]), st_next, p(work), stream))
    torch.cuda.synchronize()
    return ws, dep, img, rays_t, state[n_iter & 1].cpu().tolist()


def test_whole_loop_on_device_state_matches_the_float64_model_loop():
    ref = C.loop_model(np.float64, 0)
    bounds = C.loop_yardstick()
    inp = C.loop_inputs()
    runs = {}
    for cap in (0, 64):
        # the model's list is empty after `iterations`; two more are issued (a ray on T_thresh may live one sample longer than the model's),
        # each of them a whole iteration on an empty list
        model = C.loop_model(np.float64, cap)
        n_iter = model['iterations'] + 2
        runs[cap] = _run_loop(cap, n_iter)
        final = runs[cap][4]
        assert final[0] == 0, (cap, final)
        assert n_iter <= final[1] < C.LOOP_MAX_STEPS, (cap, final, model['steps'])   # every iteration marches at least one step; the cut never binds
    # chunking independence: a ray's samples and their compositing order do not depend on n_step
    for a, b in zip(runs[0][:3], runs[64][:3]):
        assert _same_bits(a, b)
    # a ray whose transmittance stays farther from T_thresh than the weights_sum bound cannot stop at another sample than the model's: it
    # gets the yardstick alone.  The others may carry one sample more or less behind the threshold: + T_thresh x (largest rgb, resp. t)
    on_threshold = ref['closest'] * C.LOOP_T_THRESH <= bounds['weights_sum'][0]
    slack = dict(weights_sum=C.LOOP_T_THRESH, image=C.LOOP_T_THRESH * 1.0, depth=C.LOOP_T_THRESH * float(inp['fars'][inp['fars'] < 1e30].max()))
    print(f'whole loop: {int(on_threshold.sum())} of {C.LOOP_N} rays come within the weights_sum bound of T_thresh')
    assert on_threshold.sum() < 0.3 * C.LOOP_N
    got = dict(zip(C.KEYS, (t.double().cpu().numpy() for t in runs[0][:3])))
    for key in C.KEYS[:3]:
        err = np.abs(got[key] - ref[key])
        err = err.max(-1) if err.ndim == 2 else err
        tol = bounds[key][0] + slack[key] * on_threshold
        print(f'whole loop {key}: kernel error {err[~on_threshold].max():.3e} off the threshold ({err.max():.3e} over all rays), float32 model error '
              f'{bounds[key][1]:.3e}, bound {bounds[key][0]:.3e}, err / bound {err[~on_threshold].max() / bounds[key][0]:.3f}')
        assert (err <= tol).all(), (key, int((err > tol).sum()), float(err.max()))
