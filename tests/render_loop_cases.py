"""Cases and references shared by tests/test_render_loop_cases.py (CPU) and tests/test_gpu_render_loop.py (GPU): the kernels of the inference
loop march_rays -> network -> composite_rays -> alive-list compaction (k_march_rays, k_composite_rays, k_compact_count / k_compact_write of
csrc/raymarching.hip and their `*_dev` entries with the loop state on the device, include/ngp_hip.h "On-device inference loop").

`loop_n_step`       the samples per ray and iteration, restated from raymarching.hip (cap 0 means 8).
`composite_model`   raymarching.cu:819-905 as a per-ray Python loop in the statement order of k_composite_rays.  At dtype=np.float64 it is the
                    DEFINITION; at np.float32 every operation is rounded to fp32 and exp is evaluated in fp32: the yardstick of the fp32
                    kernel's rounding (the role prefix_form / closed_form have in composite_geo_cases / composite_features_cases).
`yardstick`         per output: 4 x (max error of the float32 model against the float64 definition on the same inputs) + 1e-7 x (largest
                    reference magnitude) -- the rule of composite_geo_cases.yardstick.
`composite_table`   one call's inputs for n_step in N_STEPS: 97 rays, 61 of them in a scattered alive list, non-zero accumulators, and the named
                    rays of NAMED (finished at k, opaque, transparent, already saturated, three rays exactly on T_thresh = 2**-7).  Every other
                    ray keeps |T / T_thresh - 1| > MARGIN at every step of the definition, so fp32 and fp64 may not disagree on any alive-list
                    entry (the three exact rays take the same branch in both formats by construction).
`multi_call_table`  the same rays through 3 consecutive calls of n_step = 4 with fresh sample rows for the survivors of each call.
`compaction_case`   alive lists of the sizes / patterns in COMPACT_SIZES / COMPACT_PATTERNS (wave and block boundaries, more than 256 blocks:
                    the second trip of k_compact_write's block-prefix loop, all dead, all alive) with valid-looking ids behind n_alive.
`LADDER`            (n_total, n_alive, cap) -> n_step.
`scene`, `fields`, `random_rays`, `loop_model`   the small synthetic scene of the marcher tests, its analytic density / colour fields and the
                    whole loop (oracle.march_rays for the samples, composite_model, numpy for the compaction)."""
import functools
import math

import numpy as np

T_THRESH = 2.0 ** -7          # of the compositor tables: a power of two, so that a ray can sit on it exactly in fp32 and in fp64
MARGIN = 1e-3
N, N_ALIVE = 97, 61
N_STEPS = (1, 2, 3, 8, 13, 64)
KEYS = ('weights_sum', 'depth', 'image', 'rays_t')
VARIANTS = ('definition', 'le', 'threshold_first')   # the last two are deliberately WRONG compositors (see composite_model)

LADDER = [(4096, 4096, 0, 1), (4096, 5000, 0, 1), (4096, 1000, 0, 4), (4096, 512, 0, 8), (4096, 100, 0, 8), (4096, 100, 64, 40),
          (4096, 10, 64, 64), (4096, 0, 0, 1), (4096, 0, 64, 1)]


def loop_n_step(n_total, n_alive, cap):
    """loop_n_step of csrc/raymarching.hip: max(min(n_total // n_alive, cap), 1), cap 0 = the reference's 8 (renderer.py:349), 1 for an
    empty list"""
    if cap == 0:
        cap = 8
    if n_alive == 0:
        return 1
    q = n_total // n_alive
    return cap if q > cap else (1 if q < 1 else q)


def rows_used(rows, n_alive, n_step):
    """the rows ngp_march_rays_dev_rows publishes: n_alive * n_step padded by the STRICT round-up of raymarching.py (a full extra 128 when
    already aligned), capped by the caller's `rows`"""
    used = n_alive * n_step
    return min(rows, used + 128 - used % 128)


# ------------------------------------------------------------------------------------------------
# the compositor
# ------------------------------------------------------------------------------------------------
def composite_model(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, ws, depth, image, dtype, exp2=False,
                    variant='definition'):
    """kernel_composite_rays (raymarching.cu:819-905), one ray after the other, in the statement order of k_composite_rays:
        d0 == 0 breaks before anything else;  T = 1 - ws, w = alpha * T, ws += w, t += d1, depth += w * t, image += w * rgb;  THEN
        `if T < T_thresh: break`;  rays_alive[n] = -1 iff the loop broke, rays_t is written only for a ray that did not break.
    dtype np.float64: the definition.  np.float32: every operation rounded to fp32, exp evaluated in fp32 (exp2=True: as
    exp2(fl32(x * log2(e))), the way __expf is evaluated by the hardware's exp2 instruction).
    variant 'le' (T <= T_thresh) and 'threshold_first' (the test before the accumulation) are the two classic mistakes: the CPU test shows
    that the tables tell them from the definition.
    -> dict: rays_alive, rays_t, weights_sum, depth, image (updated COPIES, at `dtype`), count [n_alive] (samples composited per list entry),
    T_seen (per list entry the transmittances that were compared with T_thresh, as float64)"""
    f = dtype
    alive = np.array(rays_alive, np.int32).copy()
    rt, W, D, I = (np.array(a, dtype=f).copy() for a in (rays_t, ws, depth, image))
    sg, rg, de = (np.asarray(a, dtype=f) for a in (sigmas, rgbs, deltas))
    sg, rg, de = sg.reshape(-1), rg.reshape(-1, 3), de.reshape(-1, 2)
    one, thresh = f(1.0), f(T_thresh)
    log2e = f(math.log2(math.e))
    count = np.zeros(n_alive, np.int64)
    T_seen = []
    for n in range(n_alive):
        index = int(alive[n])
        t, w_sum, d = rt[index], W[index], D[index]
        r, g, b = I[index]
        seen = []
        step = 0
        while step < n_step:
            s = n * n_step + step
            d0 = de[s, 0]
            if d0 == 0:
                break
            x = f(-sg[s]) * d0
            alpha = one - (np.exp2(f(x * log2e)) if exp2 else np.exp(x))
            T = one - w_sum
            seen.append(float(T))
            if variant == 'threshold_first' and T < thresh:
                break
            w = alpha * T
            w_sum = w_sum + w
            t = t + de[s, 1]
            d = d + w * t
            r, g, b = r + w * rg[s, 0], g + w * rg[s, 1], b + w * rg[s, 2]
            count[n] += 1
            if (T <= thresh) if variant == 'le' else (T < thresh):
                break
            step += 1
        if step < n_step:
            alive[n] = -1
        else:
            rt[index] = t
        W[index], D[index] = w_sum, d
        I[index] = (r, g, b)
        T_seen.append(seen)
    assert all(a.dtype == f for a in (rt, W, D, I))
    return dict(rays_alive=alive, rays_t=rt, weights_sum=W, depth=D, image=I, count=count, T_seen=T_seen)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _rows(rng, n, n_step):
    """ordinary sample rows for n list entries: per ray an optical depth per sample drawn log-uniformly from [1e-3, 1] -> (sigmas, rgbs, deltas)"""
    tau = np.exp(rng.uniform(math.log(1e-3), 0.0, n))[:, None] * rng.uniform(0.5, 1.5, (n, n_step))
    deltas = np.stack([rng.uniform(0.005, 0.05, (n, n_step)), rng.uniform(0.005, 0.05, (n, n_step))], -1)
    sigmas = tau / deltas[..., 0]
    rgbs = rng.uniform(0.0, 1.0, (n, n_step, 3))
    return _f32(sigmas), _f32(rgbs), _f32(deltas)


def margin_violations(T_seen, exempt_first=(), T_thresh=T_THRESH):
    """list entries with a compared transmittance inside MARGIN of T_thresh (relative); for the entries in `exempt_first` (the rays that sit
    on the threshold ON PURPOSE with their first sample) only the samples after the first count"""
    bad = []
    for n, seen in enumerate(T_seen):
        seen = seen[1:] if n in exempt_first else seen
        if any(abs(T / T_thresh - 1.0) <= MARGIN for T in seen):
            bad.append(n)
    return bad


def _keep_off_threshold(call, exempt_first=()):
    """scale the sigmas of any list entry that comes within MARGIN of T_thresh (3 % per round, re-rounded to fp32) until none does: a condition
    on the INPUTS, re-checked from scratch by the CPU test"""
    for _ in range(100):
        out = composite_model(call['n_alive'], call['n_step'], call['T_thresh'], call['rays_alive'], call['rays_t'], call['sigmas'], call['rgbs'],
                              call['deltas'], call['weights_sum'], call['depth'], call['image'], np.float64)
        bad = margin_violations(out['T_seen'], exempt_first, call['T_thresh'])
        if not bad:
            return call
        for n in bad:
            call['sigmas'][n] = _f32(call['sigmas'][n].astype(np.float64) * 1.03)
    raise AssertionError('the table could not be moved off the threshold')


def named(n_step):
    """name -> position in the alive list.  'finished at k': deltas[k:] == 0, for every k in 0..n_step while n_step <= 8, else k in
    {0, 1, n_step - 1}"""
    ks = range(n_step + 1) if n_step <= 8 else (0, 1, n_step - 1)
    names = [f'finished at {k}' for k in ks] + ['opaque', 'transparent', 'already saturated', 'on the threshold', 'one ulp below the threshold',
                                                'half the threshold']
    return {name: 2 + 3 * i for i, name in enumerate(names)}    # scattered over the list, ordinary rays in between


EXACT = ('on the threshold', 'one ulp below the threshold', 'half the threshold')


@functools.lru_cache(maxsize=None)
def composite_table(n_step):
    """-> dict of one call's inputs (float32 / int32 numpy arrays; treat as read-only): n_alive, n_step, T_thresh, rays_alive [61] (a
    permutation prefix of 0..96), outside [36] (the ids that are not in the list), rays_t / weights_sum / depth [97], image [97,3], sigmas
    [61, n_step], rgbs [61, n_step, 3], deltas [61, n_step, 2], names (name -> list position)"""
    rng = np.random.default_rng(1000 + n_step)
    perm = rng.permutation(N).astype(np.int32)
    alive, outside = perm[:N_ALIVE].copy(), perm[N_ALIVE:].copy()
    sigmas, rgbs, deltas = _rows(rng, N_ALIVE, n_step)
    ws0 = _f32(rng.uniform(0.0, 0.9, N))
    depth0, image0, t0 = _f32(rng.uniform(0.1, 2.0, N)), _f32(rng.uniform(0.05, 1.0, (N, 3))), _f32(rng.uniform(0.2, 3.0, N))
    names = named(n_step)
    assert max(names.values()) < N_ALIVE
    for n in range(0, N_ALIVE, 9):          # a few ordinary rays arrive below the threshold: they stop after one sample whatever n_step is
        if n not in names.values():
            ws0[alive[n]] = np.float32(rng.uniform(0.993, 0.9999))
    for name, n in names.items():
        i = alive[n]
        if name.startswith('finished at '):
            k = int(name.split()[-1])
            deltas[n, k:] = 0.0
            sigmas[n] = _f32(1.0 / n_step / np.maximum(deltas[n, :, 0], 0.005))   # optical depth 1 over the call: the ray ends with its samples, not on T_thresh
            ws0[i] = np.float32(0.25)
        elif name == 'opaque':
            sigmas[n] = _f32(20.0 / deltas[n, :, 0].astype(np.float64))       # sigma * d0 = 20
            ws0[i] = np.float32(0.125)
        elif name == 'transparent':
            sigmas[n] = 0.0
            ws0[i] = np.float32(0.5)
        elif name == 'already saturated':
            ws0[i] = np.float32(0.9995)
        elif name == 'on the threshold':
            ws0[i] = np.float32(1.0 - 2.0 ** -7)                              # T == T_thresh: not <, the ray continues
        elif name == 'one ulp below the threshold':
            ws0[i] = np.nextafter(np.float32(1.0 - 2.0 ** -7), np.float32(1.0))
        elif name == 'half the threshold':
            ws0[i] = np.float32(1.0 - 2.0 ** -8)
        if name in EXACT or name == 'already saturated':
            sigmas[n] = _f32(0.7 / deltas[n, :, 0].astype(np.float64))        # alpha = 0.5: the sample behind the threshold is far below it
    call = dict(n_alive=N_ALIVE, n_step=n_step, T_thresh=T_THRESH, rays_alive=alive, outside=outside, rays_t=t0, weights_sum=ws0, depth=depth0,
                image=image0, sigmas=sigmas, rgbs=rgbs, deltas=deltas, names=names)
    return _keep_off_threshold(call, exempt_first={names[e] for e in EXACT})


def run_model(call, dtype, **kw):
    return composite_model(call['n_alive'], call['n_step'], call['T_thresh'], call['rays_alive'], call['rays_t'], call['sigmas'], call['rgbs'],
                           call['deltas'], call['weights_sum'], call['depth'], call['image'], dtype, **kw)


@functools.lru_cache(maxsize=None)
def table_reference(n_step):
    """the float64 definition on composite_table(n_step), computed once"""
    return run_model(composite_table(n_step), np.float64)


def bound_of(ref, f32):
    """the tolerance rule -> {key: (bound, float32 model error)}"""
    out = {}
    for key in KEYS:
        err = float(np.abs(f32[key].astype(np.float64) - ref[key]).max())
        out[key] = (4.0 * err + 1e-7 * float(np.abs(ref[key]).max()), err)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(n_step, exp2=False):
    """{key: (bound, float32 model error)} of composite_table(n_step)"""
    return bound_of(table_reference(n_step), run_model(composite_table(n_step), np.float32, exp2=exp2))


# ------------------------------------------------------------------------------------------------
# three consecutive calls
# ------------------------------------------------------------------------------------------------
MULTI_CALLS, MULTI_N_STEP = 3, 4


@functools.lru_cache(maxsize=None)
def multi_call_table():
    """-> list of 3 calls (dicts like composite_table's; call 0 IS composite_table(4)): between calls the list is compacted with numpy and the
    survivors get fresh sample rows (every 5th survivor's samples end after two); each call reads the float64 definition's state after the
    previous one.  calls[i]['rays_alive'] is the list the definition hands to call i."""
    rng = np.random.default_rng(77)
    first = composite_table(MULTI_N_STEP)
    calls = [first]
    state = run_model(first, np.float64)
    for _ in range(1, MULTI_CALLS):
        alive = state['rays_alive'][state['rays_alive'] >= 0]
        sigmas, rgbs, deltas = _rows(rng, len(alive), MULTI_N_STEP)
        deltas[::5, 2:] = 0.0
        call = dict(n_alive=len(alive), n_step=MULTI_N_STEP, T_thresh=T_THRESH, rays_alive=alive, sigmas=sigmas, rgbs=rgbs, deltas=deltas,
                    rays_t=state['rays_t'], weights_sum=state['weights_sum'], depth=state['depth'], image=state['image'])
        calls.append(_keep_off_threshold(call))
        state = run_model(call, np.float64)
    return calls


def run_multi(dtype, **kw):
    """the three calls at `dtype`, each on the previous call's outputs AT THAT dtype -> (end state, [alive list after each call])"""
    calls = multi_call_table()
    state = {k: calls[0][k].astype(dtype) for k in KEYS}
    lists = []
    for call in calls:
        out = run_model(dict(call, **state), dtype, **kw)
        state = {k: out[k] for k in KEYS}
        lists.append(out['rays_alive'])
    return state, lists


@functools.lru_cache(maxsize=None)
def multi_yardstick(exp2=False):
    """-> (float64 end state, [alive lists], {key: (bound, float32 model error)})"""
    ref, lists = run_multi(np.float64)
    f32, _ = run_multi(np.float32, exp2=exp2)
    return ref, lists, bound_of(ref, f32)


# ------------------------------------------------------------------------------------------------
# compaction
# ------------------------------------------------------------------------------------------------
COMPACT_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 65536, 65537, 70001, 640000)
COMPACT_PATTERNS = ('all alive', 'all dead', 'alternating', 'bernoulli', '1 in 1000', 'only the first', 'only the last', 'lane 63 of every wave',
                    'thread 255 of every block')
TAIL, FILL = 300, -7


def compaction_case(n, pattern, length=None):
    """-> (list [max(n + 300, length)] int32, expected survivors): the first n entries are a random permutation of 0..n-1 with the dead ones
    replaced by -1 (order matters), everything behind them holds valid-looking non-negative ids that must be ignored"""
    rng = np.random.default_rng(n * 16 + COMPACT_PATTERNS.index(pattern))
    pos = np.arange(n)
    keep = {'all alive': np.ones(n, bool), 'all dead': np.zeros(n, bool), 'alternating': pos % 2 == 0, 'bernoulli': rng.random(n) < 0.5,
            '1 in 1000': pos % 1000 == 999, 'only the first': pos == 0, 'only the last': pos == n - 1, 'lane 63 of every wave': pos % 64 == 63,
            'thread 255 of every block': pos % 256 == 255}[pattern]
    ids = rng.permutation(n).astype(np.int32)
    ids[~keep] = -1
    total = max(n + TAIL, length or 0)
    a = np.concatenate([ids, 1_000_000 + np.arange(total - n)]).astype(np.int32)
    return a, a[:n][a[:n] >= 0].copy()


# ------------------------------------------------------------------------------------------------
# the scene of the marcher tests and the whole loop
# ------------------------------------------------------------------------------------------------
def random_rays(N, seed, radius=3.2, spread=0.6):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(N, 3))
    o = (radius * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    t = rng.uniform(-spread, spread, size=(N, 3))
    d = t - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def scene(bound, cascade, seed=0, fill=0.05):
    import oracle
    import synthetic_scene as sc
    if bound == 1 and cascade == 1:
        grid = sc.occupancy_density()
        return oracle.packbits(grid, 10.0)
    rng = np.random.default_rng(seed)
    # blocky random occupancy so that rays see runs of occupied and empty voxels in every cascade
    coarse = rng.uniform(size=(cascade, 16, 16, 16)) < fill * 3
    g = np.repeat(np.repeat(np.repeat(coarse, 8, 1), 8, 2), 8, 3).reshape(cascade, -1).astype(np.float32)
    return oracle.packbits(g, 0.5)


def fields(xyzs):
    sig = (25.0 * np.exp(-3.0 * (xyzs ** 2).sum(-1)) + 2.0 * (xyzs[:, 0] > 0.2)).astype(np.float32)
    rgb = (0.5 + 0.5 * np.sin(3.0 * xyzs + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    return sig, rgb


def fields64(xyzs):
    """`fields` evaluated in float64 and rounded once to fp32 (what the GPU test computes with float64 torch ops on the device: a correctly
    rounded fp32 value up to the last bit of a double, so that host and device feed their compositors the same numbers)"""
    x = np.asarray(xyzs, np.float64)
    sig = 25.0 * np.exp(-3.0 * (x ** 2).sum(-1)) + 2.0 * (x[:, 0] > 0.2)
    rgb = 0.5 + 0.5 * np.sin(3.0 * x + np.array([0.0, 1.0, 2.0]))
    return sig.astype(np.float32), rgb.astype(np.float32)


# (T_thresh crosses the ABI as a float: the definition compares with that fp32 value, as the kernel and the oracle do)
LOOP_N, LOOP_T_THRESH, LOOP_MAX_STEPS, LOOP_SEED = 2000, float(np.float32(1e-4)), 1 << 20, 31


@functools.lru_cache(maxsize=None)
def loop_inputs():
    import oracle
    bits = scene(1.0, 1)
    o, d = random_rays(LOOP_N, LOOP_SEED)
    nears, fars = oracle.near_far_from_aabb(o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32), 0.2)
    return dict(bits=bits, o=o, d=d, nears=nears, fars=fars)


@functools.lru_cache(maxsize=None)
def loop_model(dtype, cap, exp2=False):
    """the whole loop on LOOP_N rays of `scene(1, 1)`: oracle.march_rays for the samples, fields64, composite_model at `dtype`, numpy for the
    compaction, loop_n_step for the chunking, until the list is empty.  rays_t is handed to the marcher as fp32: it IS an fp32 quantity, the
    sum of the marcher's own differences t_k - t_(k-1), which is exact in both formats (`t_exact` records that).
    -> dict: weights_sum, depth, image, rays_t, iterations, steps (sum of n_step), count [N] (samples composited per ray), closest [N] (the
    smallest |T / T_thresh - 1| among the transmittances the ray compared with T_thresh; inf for a ray without a sample), t_exact"""
    import oracle
    inp = loop_inputs()
    N_ = LOOP_N
    state = dict(weights_sum=np.zeros(N_, dtype), depth=np.zeros(N_, dtype), image=np.zeros((N_, 3), dtype), rays_t=inp['nears'].astype(dtype))
    alive = np.arange(N_, dtype=np.int32)
    count = np.zeros(N_, np.int64)
    closest = np.full(N_, np.inf)
    iterations = steps = 0
    t_exact = True
    while len(alive):
        n_alive = len(alive)
        n_step = loop_n_step(N_, n_alive, cap)
        rt32 = state['rays_t'].astype(np.float32)
        t_exact = t_exact and bool((rt32.astype(np.float64) == state['rays_t'].astype(np.float64)).all())
        x, _, de = oracle.march_rays(n_alive, n_step, alive, rt32, inp['o'], inp['d'], 1.0, inp['bits'], 1, 128, inp['nears'], inp['fars'],
                                     np.zeros(n_alive, np.float32))
        sig, rgb = fields64(x)
        out = composite_model(n_alive, n_step, LOOP_T_THRESH, alive, state['rays_t'], sig, rgb, de, state['weights_sum'], state['depth'],
                              state['image'], dtype, exp2=exp2)
        count[alive] += out['count']
        for i, seen in zip(alive, out['T_seen']):
            if seen:
                closest[i] = min(closest[i], min(abs(T / LOOP_T_THRESH - 1.0) for T in seen))
        state = {k: out[k] for k in KEYS}
        alive = out['rays_alive'][out['rays_alive'] >= 0]
        iterations += 1
        steps += n_step
    return dict(state, iterations=iterations, steps=steps, count=count, closest=closest, t_exact=t_exact)


@functools.lru_cache(maxsize=None)
def loop_yardstick(exp2=False):
    """{key: (bound, float32 model error)} of the loop's end state: the rule of `yardstick`, the float32 error taken over the rays that
    composite the same number of samples in both formats (a ray that sits on T_thresh may stop one sample apart: the GPU test grants that
    separately, per ray)"""
    ref, f32 = loop_model(np.float64, 0), loop_model(np.float32, 0, exp2)
    same = ref['count'] == f32['count']
    out = {}
    for key in KEYS:
        err = float(np.abs(f32[key].astype(np.float64) - ref[key])[same].max())
        out[key] = (4.0 * err + 1e-7 * float(np.abs(ref[key]).max()), err)
    return out
