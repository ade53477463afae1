"""Inputs for the grid backward whose sums are EXACT (tests/test_grid_lattice_cases.py on the CPU, tests/test_gpu_grid_backward_runs.py
on the GPU).  numpy + oracle only: nothing here touches a GPU.

A rounding tolerance hides a dropped contribution, so the inputs are chosen to have no rounding at all:
  * S = 0: every level has scale = H - 1, and H - 1 is a power of two;
  * points sit on the lattice x = k / (sub * (H - 1)): fma(x, scale, 0.5 | 0) is exact and the fractions are multiples of 1 / sub
    (sub = 2: {0, 1/2}, which smoothstep maps to themselves; sub = 4: linear interpolation only);
  * gradients are j * 2^-6 with small integers j.
Every contribution is then an integer multiple of unit = 2^-6 / sub^D, and every partial sum -- in any order, merged into runs or
not -- is exact in the table type as long as sum|contribution| / unit per entry stays below 2^11 (fp16) or 2^24 (fp32).  The kernel's
output must equal the float64 oracle bit for bit.

The sample sequence is a lattice walk (stay 0.55 / one lattice step 0.40 / jump 0.05, 5 % out-of-range samples, 5 % zero gradients)
with planted structure, each item an edge of the segmented wave scan of the atomic backward (corner_runs in csrc/gridencoder.hip):
  * one stretch of 130 identical points with |j| = 1 (longer than a wave holds in any lane layout: 32 point slots at 2 lanes per
    point, 4 at 16), starting at an index that is 5 mod 64;
  * runs of exactly 8, 9, 16, 17 and 32 samples inside one cell, starting at an index that is 0 and 7 mod 8 (a DPP row holds 8 samples
    at 2 lanes per point);
  * runs interrupted in the middle by one out-of-range sample (of either kind) and by one sample whose gradient is exactly zero;
  * for C > 1 runs with a sample whose gradient is zero in channel 0 only, and in channels 0 and 1 only (C >= 4): liveness is per lane;
  * two different vertices that collide in the level's table, visited alternately (equal address counts as a run);
  * x = 0 and x = 1 in every coordinate, nextafter(1, 2) and -1e-7 in one coordinate;
  * a tail: B is not a multiple of 64.
`exactness` states, from the oracle alone, what every case must satisfy; tests/test_grid_lattice_cases.py asserts it for every case
the GPU tests use, so a vacuous case fails instead of passing."""
import collections
import copy
import functools
import itertools

import numpy as np

import oracle

PREFILL = 0.25                       # the exactly representable value the "+=" runs start from
H_FOR_D = {2: 33, 3: 17, 4: 9, 5: 5}
B_SMALL = 4096 + 37
B_SORT = 16384 + 37                  # at least BIN_MIN_SAMPLES: the record-sort launch
OOB_HI, OOB_LO = 1, 2                # nextafter(1, 2) | -1e-7 in one coordinate

Case = collections.namedtuple('Case', 'D C dtype H sub gridtype align interp level_sizes B jmax seed')


def lanes_per_point(dtype, C):
    """BwdLanes<T, C>::LPP"""
    cpl = 2 if dtype == 'f16' and C % 2 == 0 else 1
    return 2 * C // cpl


def merge_kind(dtype, C):
    """3: the DPP scan (two lanes per point), 1: __shfl_up"""
    return 3 if lanes_per_point(dtype, C) == 2 else 1


def make_case(D, C, dtype, gridtype=0, align=False, interp=0, level_sizes=(1024,), B=B_SMALL, H=None, seed=0):
    H = H_FOR_D[D] if H is None else H
    assert (H - 1) & (H - 2) == 0, 'H - 1 is a power of two'
    sub = 4 if dtype == 'f32' and interp == 0 else 2
    jmax = 4 if dtype == 'f32' else (1 if D == 5 else 2)
    return Case(D, C, dtype, H, sub, gridtype, bool(align), interp, tuple(int(s) for s in level_sizes), B, jmax, seed)


def dense_size(D, H, align):
    n = (H if align else H + 1) ** D
    return (n + 7) // 8 * 8


def unit_of(case):
    return 2.0 ** -6 / case.sub ** case.D


def cap_of(case):
    return 2 ** 11 if case.dtype == 'f16' else 2 ** 24


def _offsets(case):
    return np.concatenate([[0], np.cumsum(case.level_sizes)]).astype(np.int32)


def _cells(case, k):
    """cell and fraction numerator (in 1 / sub) of lattice coordinates k"""
    t = k if case.align else k + case.sub // 2
    return t // case.sub, t % case.sub


def _lattice_point(case, cell, f):
    t = np.asarray(cell) * case.sub + np.asarray(f)
    return t if case.align else t - case.sub // 2


def _to_x(case, k):
    return (np.asarray(k, np.float64) / (case.sub * (case.H - 1))).astype(np.float32)


def _colliding_pair(case, rng, level):
    """two lattice points on vertices (every fraction 0: all the weight on the cell's lower vertex) of different cells whose lower vertices
    share the table address at `level` and the parity of every coordinate (the slot of the run merge), or None"""
    D, H = case.D, case.H
    lo = 0 if case.align else 1
    n = H - 1
    if n ** D <= 20000:
        cells = np.array(list(itertools.product(range(lo, lo + n), repeat=D)))
    else:
        cells = rng.integers(lo, lo + n, (60000, D))
    k = _lattice_point(case, cells, 0)
    idx = oracle.grid_corner_indices(_to_x(case, k), np.array([0, case.level_sizes[level]], np.int32), 0.0, H, case.gridtype, case.align)[0, :, 0].astype(np.int64)
    key = idx * (1 << D) + ((cells & 1) << np.arange(D)).sum(1)
    order = np.argsort(key, kind='stable')
    for a, b in zip(order[:-1], order[1:]):
        if key[a] == key[b] and not np.array_equal(cells[a], cells[b]):
            return k[a], k[b]
    return None


@functools.lru_cache(maxsize=None)
def _walk(case):
    """the sample sequence of a case: x [B, D] float32, the gradient numerators J [B, C] and the generator behind them"""
    D, C, H, sub, jmax = case.D, case.C, case.H, case.sub, case.jmax
    rng = np.random.default_rng(1000 + case.seed)
    N = sub * (H - 1)
    K, J, OOB = [], [], []
    pos = rng.integers(0, N + 1, D)

    def emit(k, j, oob=0):
        K.append(np.array(k, np.int64))
        J.append(np.array(j, np.int64))
        OOB.append(oob)

    def some_j(nonzero=False):
        j = rng.integers(-jmax, jmax + 1, C)
        if nonzero:
            j = np.where(j == 0, 1, j)
        return j

    def walk(n=1):
        nonlocal pos
        for _ in range(n):
            u = rng.random()
            if u >= 0.95:
                pos = rng.integers(0, N + 1, D)
            elif u >= 0.55:
                pos = pos.copy()
                d = rng.integers(D)
                pos[d] = min(N, max(0, pos[d] + (1 if rng.random() < 0.5 else -1)))
            v = rng.random()
            j = some_j()
            if not j.any():
                j[rng.integers(C)] = rng.choice([-1, 1])   # whole-sample zeros are the 5 % below, no more
            emit(pos, j if v >= 0.05 else np.zeros(C, np.int64), 0 if rng.random() >= 0.05 else (OOB_HI if len(K) & 1 else OOB_LO))

    def pad_to(m, r):
        while len(K) % m != r:
            walk()

    # cells far from one another (odd coordinates: no shared vertex) with every fraction available in both align modes
    per_axis = (H - 1) // 2
    picks = rng.choice(per_axis ** D, size=min(per_axis ** D, 64), replace=False)
    far = [[1 + 2 * ((int(p) // per_axis ** d) % per_axis) for d in range(D)] for p in picks]
    far_it = itertools.cycle(far)

    def in_cell(cell):
        return _lattice_point(case, cell, rng.integers(0, sub, D))

    def run(n, j_of=None, interrupt=None):
        cell = next(far_it)
        for i in range(n):
            j = some_j(nonzero=True) if j_of is None else j_of(i)
            if interrupt is not None and i == n // 2:
                interrupt(in_cell(cell))
            else:
                emit(in_cell(cell), j)

    emit(np.zeros(D), some_j(True))          # x = 0 and x = 1 in every coordinate
    emit(np.full(D, N), some_j(True))
    walk(70)
    pad_to(64, 5)
    stretch = _lattice_point(case, next(far_it), np.full(D, sub // 2))   # every fraction 1/2: all 2^D corners carry weight
    for _ in range(130):
        emit(stretch, rng.choice([-1, 1], C))
    for start in (0, 7):
        for n in (8, 9, 16, 17, 32):
            pad_to(8, start)
            run(n)
    walk(3)
    run(25, interrupt=lambda k: emit(k, some_j(True), OOB_HI))
    run(25, interrupt=lambda k: emit(k, some_j(True), OOB_LO))
    run(25, interrupt=lambda k: emit(k, np.zeros(C)))
    if C > 1:
        def zero_first(nz):
            def j_of(i):
                j = some_j(nonzero=True)
                if i in (7, 12):
                    j[:nz] = 0
                return j
            return j_of
        run(25, j_of=zero_first(1))
        if C >= 4:
            run(25, j_of=zero_first(2))
    for level in range(len(case.level_sizes)):   # (S = 0: every level has the same scale, so a level is indexed like a table of its own)
        pair = _colliding_pair(case, rng, level)
        if pair is not None:
            for i in range(24):
                emit(pair[i & 1], some_j(nonzero=True))
    assert len(K) <= case.B - 64, 'planted structure must leave room for the walk'
    walk(case.B - len(K))

    K, J, OOB = np.array(K), np.array(J), np.array(OOB)
    x = _to_x(case, K)
    sel = np.flatnonzero(OOB)
    axis = sel % D
    x[sel, axis] = np.where(OOB[sel] == OOB_HI, np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(-1e-7))
    x.setflags(write=False)
    return x, J, rng


def points(case):
    """x [B, D] float32, offsets int32 [L + 1], S = 0.0: the points of make(case) without its gradients (the forward's cases,
    tests/grid_forward_cases.py)"""
    return _walk(case)[0], _offsets(case), 0.0


@functools.lru_cache(maxsize=None)
def make(case):
    """x [B, D] float32, g [L, B, C] float32, offsets int32 [L + 1], S = 0.0 (cached: treat the arrays as read-only)"""
    x, J, rng = _walk(case)
    rng = copy.deepcopy(rng)
    C, H = case.C, case.H
    L = len(case.level_sizes)
    g = np.empty((L, case.B, C), np.float32)
    g[0] = J * 2.0 ** -6
    for l in range(1, L):            # same structure on every level, other signs
        g[l] = g[0] * rng.choice([-1.0, 1.0], (case.B, 1))
    offs = _offsets(case)
    # a small level cannot take every sample's contribution below the cap: its gradient is zero behind a window (the planted runs are in front)
    window = [case.B] * L
    while True:
        A, _ = oracle.grid_backward(np.abs(g), x, offs, int(offs[-1]), C, 0.0, H, gridtype=case.gridtype, align_corners=case.align,
                                    interp=case.interp)
        over = [l for l in range(L) if (PREFILL + A[offs[l]:offs[l + 1]].max()) / unit_of(case) >= 0.75 * cap_of(case)]
        if not over:
            break
        for l in over:
            assert l > 0 and window[l] > 256, 'level 0 carries the planted structure whole: shrink |j| or the stretch instead'
            window[l] //= 2
            g[l, window[l]:] = 0.0
    for a in (g, offs):
        a.setflags(write=False)
    return x, g, offs, 0.0


def entry_hits(x, offs, S, H, gridtype, align):
    """per table entry: how many corners of in-range samples address it"""
    idx = oracle.grid_corner_indices(x, offs, S, H, gridtype, align)
    hits = np.zeros(int(offs[-1]), np.int64)
    for l in range(len(offs) - 1):
        row = idx[l].reshape(-1)
        row = row[row != 0xFFFFFFFF].astype(np.int64)
        hits[offs[l]:offs[l + 1]] = np.bincount(row, minlength=int(offs[l + 1] - offs[l]))
    return hits, idx


@functools.lru_cache(maxsize=None)
def exactness(case):
    """what the oracle alone says about a case (see the module docstring)"""
    x, g, offs, S = make(case)
    D, C, H = case.D, case.C, case.H
    kw = dict(gridtype=case.gridtype, align_corners=case.align, interp=case.interp)
    n = int(offs[-1])
    ref, _ = oracle.grid_backward(g, x, offs, n, C, S, H, **kw)
    A, _ = oracle.grid_backward(np.abs(g), x, offs, n, C, S, H, **kw)
    hits, idx = entry_hits(x, offs, S, H, case.gridtype, case.align)
    inside = idx[0, :, 0] != 0xFFFFFFFF
    zero = inside & ~np.any(g[0] != 0, axis=1)
    live = inside & ~zero
    # runs at level 0: consecutive live samples with the same 2^D addresses (a run in every slot of the merge)
    same = live[1:] & live[:-1] & np.all(idx[0, 1:] == idx[0, :-1], axis=1)
    edges = np.flatnonzero(~same)
    runs = np.diff(np.concatenate([[-1], edges, [case.B - 1]]))
    # and as the merge sees them: slot p of a sample holds the vertex whose coordinates have the parities p, so neighbouring cells that
    # share a vertex continue its run.  One list of run lengths per parity class.
    k_all = np.rint(np.where(inside[:, None], x, 0).astype(np.float64) * (case.sub * (H - 1))).astype(np.int64)
    cell_all, _ = _cells(case, k_all)
    vertex_runs = []
    for p in range(1 << D):
        corner_of = ((((p >> np.arange(D)) & 1) ^ (cell_all & 1)) << np.arange(D)).sum(1)
        addr = idx[0, np.arange(case.B), corner_of]
        cont = live[1:] & live[:-1] & (addr[1:] == addr[:-1])
        vertex_runs.append(np.diff(np.concatenate([[-1], np.flatnonzero(~cont), [case.B - 1]])))
    mid = np.arange(1, case.B - 1)
    bridged = live[mid - 1] & live[mid + 1] & np.all(idx[0, mid - 1] == idx[0, mid + 1], axis=1)
    # distinct vertices sharing a table address, per level
    in_x = x[inside].astype(np.float64) * (case.sub * (H - 1))
    cell, _ = _cells(case, np.rint(in_x).astype(np.int64))
    corner = (np.arange(1 << D)[:, None] >> np.arange(D)) & 1
    vcode = ((cell[:, None, :] + corner[None]) * (H + 2) ** np.arange(D)).sum(-1).reshape(-1)
    collisions = []
    for l in range(len(offs) - 1):
        pairs = np.unique(np.stack([idx[l][inside].reshape(-1).astype(np.int64), vcode], 1), axis=0)
        collisions.append(int((np.bincount(pairs[:, 0]) > 1).sum()))
    return dict(ref=ref, A=A, hits=hits, unit=unit_of(case), cap=cap_of(case), runs=runs, vertex_runs=vertex_runs, inside=inside, lattice=in_x,
                dead_in_run=int((bridged & ~inside[mid]).sum()), zero_in_run=int((bridged & zero[mid]).sum()),
                partial_zero_in_run=int((bridged & live[mid] & np.any(g[0, mid] == 0, axis=1)).sum()), collisions=collisions)


def hashed_levels(case):
    return [l for l, s in enumerate(case.level_sizes) if case.gridtype == 0 and (case.H if case.align else case.H + 1) ** case.D > s]


# ---------------------------------------------------------------------------------------------------------------------
# the case tables of tests/test_gpu_grid_backward_runs.py
# ---------------------------------------------------------------------------------------------------------------------
def _mode(i, D, H):
    """index modes in rotation: hash with collisions | dense + smoothstep | tiled, wrapping (size no power of two) | hash + align_corners
    | hash + smoothstep | tiled, wrapping (power of two) + align_corners"""
    return [dict(gridtype=0, level_sizes=(1024,)),
            dict(gridtype=0, level_sizes=(dense_size(D, H, False),), interp=1),
            dict(gridtype=1, level_sizes=(1000,)),
            dict(gridtype=0, level_sizes=(1024,), align=True),
            dict(gridtype=0, level_sizes=(1024,), interp=1),
            dict(gridtype=1, level_sizes=(512,), align=True)][i % 6]


def _layout_cases():
    """(a) all 32 instantiations; the mode index counts inside each (dtype, merge kind) group so that every group sees every mode it has
    room for (fp32 with the DPP merge is C = 1 alone: four cases, the first four modes -- they hold all five features)"""
    out, count = [], collections.Counter()
    for dtype in ('f16', 'f32'):
        for C in (1, 2, 4, 8):
            for D in (2, 3, 4, 5):
                grp = (dtype, merge_kind(dtype, C))
                out.append(make_case(D, C, dtype, seed=len(out), **_mode(count[grp], D, H_FOR_D[D])))
                count[grp] += 1
    return out


LAYOUT_CASES = _layout_cases()

# (b) three levels of one scale and three sizes: hashed (tiled: wrapping) | dense | tiny
SWEEP_CASES = [make_case(3, 2, dtype, gridtype=gt, align=al, interp=ip, level_sizes=(1024, dense_size(3, 17, al), 8), seed=100 + i)
               for dtype in ('f32', 'f16') for i, (gt, al, ip) in enumerate(itertools.product((0, 1), (False, True), (0, 1)))]

# (c) the in-kernel input mapping, bound = 2
BOUND = 2.0
MAPPED_CASES = [make_case(3, 2, 'f32', level_sizes=(1024,), seed=200), make_case(3, 4, 'f16', level_sizes=(1024,), interp=1, seed=201)]

# (d) atomic levels riding in the record-sort launch: (D, gridtype, H, sizes); which branch of plan_backward the large level takes:
#   D = 3, hash,  H = 129, 2^22: 130^3 <= 2^22, so the level is indexed DENSE, not interleaved (> 128 * 4096), 1024 slices > BIN_MAX_BINS -> atomic
#   D = 3, tiled, H = 129, 2^20: 130^3 >  2^20, TILED with wrapping (index % size), neither hashed nor interleaved                -> atomic
#   D = 2, hash,  H = 2049, 2^22: 2050^2 > 2^22, so the level is HASHED, 1024 slices > BIN_MAX_BINS                                 -> atomic
# the 4096-entry level is binned in all three (hashed: one slice; tiled: round-robin bins)
SORT_LAUNCH_CASES = [make_case(D, 2, 'f16', gridtype=gt, level_sizes=sizes[::order], B=B_SORT, H=H, seed=300 + 2 * i + (order < 0))
                     for i, (D, gt, H, sizes) in enumerate([(3, 0, 129, (4096, 1 << 22)), (3, 1, 129, (4096, 1 << 20)),
                                                            (2, 0, 2049, (4096, 1 << 22))])
                     for order in (1, -1)]

ALL_CASES = LAYOUT_CASES + SWEEP_CASES + MAPPED_CASES + SORT_LAUNCH_CASES


def case_id(case):
    return '%s-C%d-D%d-H%d-%s%s%s-%s' % (case.dtype, case.C, case.D, case.H, 'tiled' if case.gridtype else 'hash', '-align' if case.align else '',
                                         '-smooth' if case.interp else '', 'x'.join(str(s) for s in case.level_sizes))


def world_coordinates(x):
    """[-2, 2] coordinates of unit lattice points, in fp32 as the kernel's InputMap undoes them: (xw + 2) * 0.25"""
    return (x * np.float32(4.0) - np.float32(2.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# (e) ray-ordered samples off the lattice, D dimensions
# ---------------------------------------------------------------------------------------------------------------------
def ray_points(n_rays, per_ray, D, rng):
    """samples ordered along rays (consecutive samples share cells on the coarse levels, like the marcher's output)"""
    o = rng.uniform(0.05, 0.95, (n_rays, 1, D))
    d = rng.normal(size=(n_rays, 1, D))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = (np.arange(per_ray)[None, :, None] + rng.uniform(0, 1, (n_rays, 1, 1))) * (np.sqrt(3) / 1024)
    return np.clip(o + d * t, 0.0, 1.0).reshape(-1, D).astype(np.float32)


RAY_CASES = [  # D, C, dtype, gridtype, align, interp, log2 of the largest level: every index mode once
    (3, 2, 'f32', 0, False, 0, 12),    # dense, dense, hashed
    (3, 8, 'f32', 1, True, 0, 10),     # tiled: dense, wrapping, wrapping; align_corners
    (5, 1, 'f32', 0, False, 1, 10),    # hashed; smoothstep
    (3, 4, 'f16', 0, True, 0, 12),     # dense, dense, hashed; align_corners
]
FP16_MIN_NORMAL = 2.0 ** -14


@functools.lru_cache(maxsize=None)
def ray_case(D, C, dtype, gridtype, align, interp, log2_size):
    """64 rays x 64 samples, 3 levels, per_level_scale 1.6, H = 8; x, g, offsets, S, H and, from the oracle, the exact sums `ref`, the
    per-entry sum|contribution| `A`, the per-entry hit counts and how many (level, sample) gradients were zeroed (fp16 only, below).

    The bound of the GPU test charges every rounding to the table type with a RELATIVE error (2^-11 in fp16).  That holds for normal numbers
    only: below 2^-14 an fp16 rounding costs up to 2^-25 absolute, whatever the value (a contribution of 1e-11 -- a corner weight of 1e-10
    next to a cell border -- is stored as 0).  So the fp16 case keeps every contribution in the normal range: |g| in [16, 32] (sums stay
    below 288 * 32, far from 65504), and the few samples with a corner weight in (0, 2^-18) at a level get a zero gradient at that level
    (skipped by the kernel like the samples behind a terminated ray).  With every |contribution| >= 2^-14, a partial sum that cancels into
    the subnormal range costs 2^-25 <= 2^-11 * A_e: the bound's model holds for every add."""
    rng = np.random.default_rng(40 + 10 * D + C)
    offs, pls = oracle.grid_offsets(input_dim=D, num_levels=3, level_dim=C, per_level_scale=1.6, base_resolution=8, log2_hashmap_size=log2_size,
                                    align_corners=align)
    S, H, n = float(np.log2(pls)), 8, int(offs[-1])
    x = ray_points(64, 64, D, rng)
    x[0], x[1], x[2] = 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))
    x[3, 0] = -1e-7
    B = x.shape[0]
    kw = dict(gridtype=gridtype, align_corners=align, interp=interp)
    zeroed = 0
    if dtype == 'f16':
        g = oracle.round_fp16(rng.uniform(16.0, 32.0, (3, B, C)) * rng.choice([-1.0, 1.0], (3, B, C)))
        one = np.ones((3, 1, 1), np.float32)
        for b in range(B):   # the sample's corner weights, per level: the oracle's backward of a unit gradient on this sample alone
            w, _ = oracle.grid_backward(one, x[b:b + 1], offs, n, 1, S, H, **kw)
            for l in range(3):
                wl = w[offs[l]:offs[l + 1]]
                if np.any((wl > 0) & (wl < FP16_MIN_NORMAL / 16.0)):
                    g[l, b] = 0.0
                    zeroed += 1
    else:
        g = rng.normal(size=(3, B, C)).astype(np.float32) * 0.05
    g[:, 1000:1100] = 0.0   # exactly-zero gradients are skipped
    ref, _ = oracle.grid_backward(g, x, offs, n, C, S, H, **kw)
    A, _ = oracle.grid_backward(np.abs(g), x, offs, n, C, S, H, **kw)
    hits, _ = entry_hits(x, offs, S, H, gridtype, align)
    for a in (x, g, offs, ref, A, hits):
        a.setflags(write=False)
    return dict(x=x, g=g, offs=offs, S=S, H=H, ref=ref, A=A, hits=hits, zeroed=zeroed)


# ---------------------------------------------------------------------------------------------------------------------
# (f) exact sums at ONE level of a table whose scales are no powers of two (tests/test_gpu_grid_backward_paths.py: the level that takes
# the atomics in a launch of the record sort)
# ---------------------------------------------------------------------------------------------------------------------
def half_lattice_coordinates(scale):
    """the float32 coordinates x in [0, 1] whose position fma(x, scale, 0.5) at a level of (float32) scale `scale` is EXACTLY a multiple of
    1/2.  x = m / (2 scale) is not representable in general; the fma's single rounding snaps most of them onto the half lattice, and the ones
    it does not are left out.  (x * scale + 0.5 is exact in float64 for a float32 x and scale: its rounding to float32 is the fma's result.)"""
    scale = np.float32(scale)
    m = np.arange(0, int(np.floor(2.0 * float(scale))) + 1)
    x = (m / (2.0 * float(scale))).astype(np.float32)
    pos = (x.astype(np.float64) * float(scale) + 0.5).astype(np.float32).astype(np.float64)
    keep = (x <= 1.0) & (pos * 2.0 == np.rint(pos * 2.0))
    return x[keep]


@functools.lru_cache(maxsize=None)
def level_lattice(B, D, scale, seed):
    """x [B, D] float32 on the half lattice of the level with this scale (every corner weight there is a multiple of 2^-D) and gradient
    numerators J [B, 2] (the gradient is J * 2^-6): a walk over the lattice as in _walk (stay / step / jump), a stretch of 130 identical
    points starting at 5 mod 64, runs of 8, 9, 16, 17 and 32 samples on one point, 5 % exactly-zero gradients, one point outside the unit cube.
    Every contribution at that level is a multiple of level_lattice_unit(D): sums in any order are exact in fp16 while they stay below the
    cap -- level_lattice_exact says whether they do."""
    rng = np.random.default_rng(7000 + seed)
    coord = half_lattice_coordinates(scale)
    n = len(coord)
    assert n >= 8
    K, J = [], []
    pos = rng.integers(0, n, D)

    def step():
        nonlocal pos
        u = rng.random()
        if u >= 0.95:
            pos = rng.integers(0, n, D)
        elif u >= 0.55:
            pos = pos.copy()
            d = rng.integers(D)
            pos[d] = min(n - 1, max(0, pos[d] + (1 if rng.random() < 0.5 else -1)))
        j = rng.integers(-2, 3, 2)
        if not j.any():
            j[rng.integers(2)] = rng.choice([-1, 1])
        K.append(pos)
        J.append(j if rng.random() >= 0.05 else np.zeros(2, np.int64))

    for _ in range(69):
        step()
    here = rng.integers(0, n, D)
    for _ in range(130):
        K.append(here)
        J.append(rng.choice([-1, 1], 2))
    for length in (8, 9, 16, 17, 32):
        while len(K) % 8 != 7:
            step()
        here = rng.integers(0, n, D)
        for _ in range(length):
            j = rng.integers(-2, 3, 2)
            K.append(here)
            J.append(np.where(j == 0, 1, j))
    while len(K) < B:
        step()
    x = coord[np.array(K[:B])]
    x[40, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))   # outside: no contribution anywhere
    J = np.array(J[:B], np.int64)
    x.setflags(write=False)
    J.setflags(write=False)
    return x, J


def level_lattice_unit(D):
    return 2.0 ** -6 / 2 ** D


def level_lattice_exact(x, g_level, offs, level, S, H, gridtype=0):
    """from the oracle alone: at `level` every sum is an integer multiple of the unit, and sum|contribution| stays below 3/4 of the fp16 cap
    (2^11 units) in every entry -- then any order of fp16 additions, merged into runs or not, gives the same bits.  Returns the largest
    sum|contribution| in units."""
    L, D = len(offs) - 1, x.shape[1]
    g = np.zeros((L,) + g_level.shape, np.float32)
    g[level] = g_level
    n = int(offs[-1])
    ref, _ = oracle.grid_backward(g, x, offs, n, 2, S, H, gridtype=gridtype)
    A, _ = oracle.grid_backward(np.abs(g), x, offs, n, 2, S, H, gridtype=gridtype)
    unit = level_lattice_unit(D)
    assert np.array_equal(ref / unit, np.rint(ref / unit)), 'a contribution off the lattice'
    assert A.max() / unit < 0.75 * 2 ** 11, 'sums leave the range in which fp16 holds every multiple of the unit'
    return A.max() / unit
