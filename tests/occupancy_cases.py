"""Models and case tables shared by tests/test_occupancy_cases.py (CPU) and tests/test_gpu_occupancy.py (GPU): the kernels that decide which
samples exist at all -- k_density_scatter / k_density_apply_mean / k_packbits behind ngp_density_grid_update and ngp_packbits_ex,
k_coarse_occupancy and k_cull_rays (csrc/raymarching.hip; include/ngp_hip.h states what each must return).

`coarse_model`          ngp_coarse_occupancy from the header's statement in numpy: unpack the bitfield, undo the Morton order, `any` over 4^3
                        blocks, OR with the 26 neighbouring blocks, flatten x fastest.  COARSE_VARIANTS[1:] are deliberately WRONG.
`cull_model`            k_cull_rays in fp32, statement by statement: oracle.cull_rays (oracle/ngp_oracle.c orc_cull_rays).  Kernel and model
                        perform the same correctly rounded fp32 operations, so their verdicts are compared without a tolerance.
                        CULL_VARIANTS[1:] are deliberately WRONG.
`density_update_model`  nerf/renderer.py:515-529 as ngp_density_grid_update states it: fp32 cell arithmetic, the exact mean.  Per cell sampled
                        more than once the SET of admissible values (any one sample may win), and the grid in which the first one wins.
                        UPDATE_VARIANTS[1:] are deliberately WRONG.
`packbits_model`        bit i of byte n = grid[8 n + i] > fminf(thresh, cap) in numpy.
`VARIANTS`              the wrong versions by family: coarse (no dilation, faces only, axes swapped), cull (step 1.8, lookup from lp, finest
                        cascade only), update (ema below zero, no decay, mean without clamp, ge packbits).

Tables: `coarse_fill` x COARSE_GRIDS, `cull_table` x CULL_CONFIGS with `NAMED_RAYS`, `update_table` x UPDATE_CELLS x UPDATE_KINDS,
`packbits_cases`.  All are deterministic, cached and to be treated as read-only."""
import functools
import math

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------
# bitfields <-> volumes
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _morton_xyz(H):
    """[H^3, 3] int: (x, y, z) of every Morton index"""
    import oracle
    return oracle.morton3D_invert(np.arange(H ** 3, dtype=np.int32)).astype(np.int64)


def unpack_volumes(bits, C, H):
    """bitfield [C * H^3 / 8] (bit i of byte n = Morton index 8 n + i) -> bool [C, z, y, x]"""
    occ = np.unpackbits(np.ascontiguousarray(bits, np.uint8), bitorder='little').reshape(C, H ** 3).astype(bool)
    xyz = _morton_xyz(H)
    vol = np.zeros((C, H, H, H), bool)
    vol[:, xyz[:, 2], xyz[:, 1], xyz[:, 0]] = occ
    return vol


def pack_volumes(vol):
    """bool [C, z, y, x] -> bitfield, the inverse of unpack_volumes"""
    C, H = vol.shape[0], vol.shape[1]
    xyz = _morton_xyz(H)
    occ = vol[:, xyz[:, 2], xyz[:, 1], xyz[:, 0]]
    return np.packbits(occ.reshape(-1), bitorder='little')


# ------------------------------------------------------------------------------------------------
# coarse occupancy
# ------------------------------------------------------------------------------------------------
COARSE_VARIANTS = ('definition', 'no dilation', 'faces only', 'axes swapped')
COARSE_GRIDS = [(H, C) for H in (16, 32, 64, 128) for C in (1, 3, 8) if C < 8 or H <= 32]
COARSE_FILLS = ('empty', 'full', 'first voxel', 'last voxel', 'odd voxel', '64 bits', 'sparse')


def coarse_model(bits, C, H, variant='definition'):
    """include/ngp_hip.h: per cascade a (H/4)^3 byte grid (x fastest), 1 when any voxel of the cell's 4^3 block or of one of its 26 neighbouring
    blocks is occupied -> uint8 [C * (H/4)^3]"""
    R = H // 4
    blocks = unpack_volumes(bits, C, H).reshape(C, R, 4, R, 4, R, 4).any(axis=(2, 4, 6))          # [C, z, y, x]
    if variant == 'no dilation':
        shifts = [(0, 0, 0)]
    elif variant == 'faces only':
        shifts = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    else:
        shifts = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    padded = np.zeros((C, R + 2, R + 2, R + 2), bool)                                              # clipped at the border: nothing outside
    padded[:, 1:-1, 1:-1, 1:-1] = blocks
    out = np.zeros_like(blocks)
    for dz, dy, dx in shifts:
        out |= padded[:, 1 + dz:R + 1 + dz, 1 + dy:R + 1 + dy, 1 + dx:R + 1 + dx]
    if variant == 'axes swapped':
        out = out.transpose(0, 3, 2, 1)                                                            # z fastest
    return np.ascontiguousarray(out).reshape(-1).astype(np.uint8)


def odd_voxel(H):
    """a voxel whose three block coordinates differ, x and z by two blocks at least (its cell is not set when two axes are swapped):
    (5, 22, 41) mod H, or (1, H/2 + 2, H - 3) where those come too close (H = 16, 32)"""
    v = (5 % H, 22 % H, 41 % H)
    return v if len({a // 4 for a in v}) == 3 and abs(v[0] // 4 - v[2] // 4) >= 2 else (1, H // 2 + 2, H - 3)


@functools.lru_cache(maxsize=None)
def coarse_fill(name, C, H):
    """-> bitfield of C cascades of H^3"""
    R = H // 4
    vol = np.zeros((C, H, H, H), bool)
    rng = np.random.default_rng(H * 100 + C * 10 + COARSE_FILLS.index(name))
    if name == 'full':
        vol[:] = True
    elif name == 'first voxel':
        vol[:, 0, 0, 0] = True
    elif name == 'last voxel':
        vol[:, H - 1, H - 1, H - 1] = True
    elif name == 'odd voxel':
        x, y, z = odd_voxel(H)
        for c in range(C):
            vol[c, z, y, (x + 4 * c) % H] = True       # (another block per cascade: a kernel that mixes the cascades up shows)
    elif name == '64 bits':
        # 64 blocks, as far apart as the grid allows (4 x 4 x 4 of them, R / 4 blocks from one to the next), block k holding only bit
        # (k + cascade) % 64 of its 64: every single bit of a block must set its cell
        s = max(R // 4, 1)
        local = _morton_xyz(4)                        # bit index inside a block -> (x, y, z) inside it: 8 consecutive bytes of the bitfield
        for c in range(C):
            for k in range(64):
                bx, by, bz = (k % 4) * s, (k // 4 % 4) * s, (k // 16) * s
                lx, ly, lz = local[(k + c) % 64]
                vol[c, bz * 4 + lz, by * 4 + ly, bx * 4 + lx] = True
    elif name == 'sparse':
        for c in range(C):
            idx = rng.integers(0, H ** 3, size=max(2, R ** 3 // 64))
            vol[c].reshape(-1)[idx] = True
    elif name != 'empty':
        raise ValueError(name)
    return pack_volumes(vol)


# ------------------------------------------------------------------------------------------------
# ray cull
# ------------------------------------------------------------------------------------------------
CULL_VARIANTS = ('definition', 'step 1.8', 'lookup from lp', 'finest cascade only')
CULL_PAIRS = [(1.0, 1), (2.0, 2), (1.5, 2), (4.0, 3), (3.0, 3), (16.0, 5)]        # (bound, cascades)
CULL_CONFIGS = [(bound, C, H) for H in (16, 32, 64) for bound, C in CULL_PAIRS]
CULL_SIZES = (1, 255, 256, 257)
CULL_N = 20000
DT_GAMMAS = (0.0, 1.0 / 128, 1.0 / 32)


def cull_model(o, d, nears, fars, bound, C, H, coarse, variant='definition'):
    import oracle
    return oracle.cull_rays(o, d, nears, fars, bound, C, H, coarse, variant=CULL_VARIANTS.index(variant))


@functools.lru_cache(maxsize=None)
def cull_grid(bound, C, H):
    """-> bitfield: per cascade a few isolated random voxels and a few voxels on the faces, edges and corners of the cascade's box.  The
    cascades are filled independently of each other (a voxel of cascade c has no counterpart in cascade c + 1), so that a lookup that
    leaves a cascade out is seen."""
    rng = np.random.default_rng(int(bound * 8) * 1000 + C * 100 + H)
    vol = np.zeros((C, H, H, H), bool)
    for c in range(C):
        for _ in range(4):
            x, y, z = rng.integers(0, H, 3)
            vol[c, z, y, x] = True
        for _ in range(6):                              # on the surface of the box: one, two or three coordinates at an end
            v = rng.integers(1, H - 1, 3)
            ends = rng.choice(3, size=rng.integers(1, 4), replace=False)
            v[ends] = rng.choice([0, H - 1], size=len(ends))
            vol[c, v[2], v[1], v[0]] = True
    return pack_volumes(vol)


def voxel_centres(bits, bound, C, H):
    """-> [K, 3] world positions of the occupied voxels' centres, [K] the size of a voxel of their cascade"""
    vol = unpack_volumes(bits, C, H)
    c, z, y, x = np.nonzero(vol)
    mb = np.minimum(2.0 ** c, bound)
    p = (np.stack([x, y, z], -1) + 0.5) / H * 2.0 - 1.0
    return p * mb[:, None], 2.0 * mb / H


@functools.lru_cache(maxsize=None)
def cull_table(bound, C, H):
    """-> dict: bits, coarse (coarse_model of bits), o, d [CULL_N, 3], nears, fars [CULL_N] fp32.  A third of the origins lie inside the
    box; 40 % of the rays are aimed at an occupied voxel with a jitter of up to two voxels (random rays alone emit too rarely on sparse
    grids), half of those passing it at a shallow angle to the nearest face of the box; 10 % have one or two direction components set to
    zero WITHOUT renormalising (axis-parallel rays among them, |d| < 1)."""
    import oracle
    rng = np.random.default_rng(int(bound * 8) * 1000 + C * 100 + H + 7)
    N = CULL_N
    bits = cull_grid(bound, C, H)
    o = rng.normal(size=(N, 3))
    o = 3.2 * bound * o / np.linalg.norm(o, axis=1, keepdims=True)
    inside = np.arange(N) % 3 == 0
    o[inside] = rng.uniform(-bound, bound, size=(int(inside.sum()), 3))
    target = rng.uniform(-0.9 * bound, 0.9 * bound, size=(N, 3))
    centres, size = voxel_centres(bits, bound, C, H)
    aimed = np.arange(N) % 5 < 2
    pick = rng.integers(0, len(centres), size=N)
    jitter = rng.uniform(-2.0, 2.0, size=(N, 3)) * size[pick][:, None]
    target[aimed] = (centres[pick] + jitter)[aimed]
    # grazing rays: through the target at a shallow angle to the box face it is nearest to, from an origin outside the box -- the short
    # chords through the corners and edges of a cascade's box, where only the lookup from the cascade below finds the voxel
    graze = aimed & (np.arange(N) % 10 < 5) & ~inside
    tg = target[graze]
    axis = np.abs(tg).argmax(axis=1)
    dirs = rng.normal(size=tg.shape)
    dirs[np.arange(len(tg)), axis] *= 0.15
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o[graze] = tg - dirs * 3.2 * bound
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(F32), d.astype(F32)
    zeroed = np.arange(N) % 10 == 7
    which = rng.integers(0, 3, size=N)
    d[zeroed, which[zeroed]] = 0.0
    two = zeroed & (np.arange(N) % 20 == 7)
    d[two, (which[two] + 1) % 3] = 0.0
    nears, fars = oracle.near_far_from_aabb(o, d, np.array([-bound] * 3 + [bound] * 3, F32), 0.2)
    return dict(bits=bits, coarse=coarse_model(bits, C, H), o=o, d=d, nears=nears, fars=fars)


def emits(table, bound, C, H, dt_gamma, first=None):
    """does the ray emit ANY sample before `far`?  oracle.march_rays with one sample slot per ray, t starting at near -> bool [N]"""
    import oracle
    N = len(table['nears']) if first is None else first
    _, _, de = oracle.march_rays(N, 1, np.arange(N, dtype=np.int32), table['nears'], table['o'], table['d'], bound, table['bits'], C, H,
                                 table['nears'], table['fars'], np.zeros(N, F32), dt_gamma=dt_gamma, max_steps=1024)
    return de[:N, 0] > 0


@functools.lru_cache(maxsize=None)
def table_emits(bound, C, H, dt_gamma):
    """`emits` of cull_table(bound, C, H), computed once"""
    return emits(cull_table(bound, C, H), bound, C, H, dt_gamma)


# name -> (fill of a (bound 1, 1 cascade, 16^3) grid, origin, direction, near, far, kept?) -- the verdicts include/ngp_hip.h states
_NAN, _INF = float('nan'), float('inf')
NAMED_GRID = (1.0, 1, 16)
NAMED_RAYS = {
    'near >= far is dropped':              ('full', (0.0, 0.0, -3.0), (0.0, 0.0, 1.0), 3.0, 3.0, False),
    'a ray that misses the box is dropped': ('full', (0.0, 0.0, -3.0), (0.0, 1.0, 0.0), FLT_MAX, FLT_MAX, False),
    'zero direction is kept':              ('empty', (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.2, 3.0, True),
    'NaN direction is kept':               ('empty', (0.0, 0.0, -3.0), (_NAN, 0.0, 1.0), 2.0, 4.0, True),
    'far = +inf is kept':                  ('empty', (0.0, 0.0, -3.0), (0.0, 0.0, 1.0), 2.0, _INF, True),
    'more than 4096 samples: kept':        ('empty', (0.0, 0.0, -3.0), (0.0, 0.0, 1.0), 0.0, 2000.0, True),
    'just under 4096 samples: judged':     ('empty', (0.0, 0.0, -3.0), (0.0, 0.0, 1.0), 0.0, 1800.0, False),
    'a ray in an empty grid is dropped':   ('empty', (0.1, 0.2, -3.0), (0.0, 0.0, 1.0), 2.0, 4.0, False),
    'a ray through a full grid is kept':   ('full', (0.1, 0.2, -3.0), (0.0, 0.0, 1.0), 2.0, 4.0, True),
}


def named_rays(fill):
    """-> names, o, d, nears, fars, kept of the NAMED_RAYS of one fill"""
    rows = [(k,) + v[1:] for k, v in NAMED_RAYS.items() if v[0] == fill]
    return ([r[0] for r in rows], np.array([r[1] for r in rows], F32), np.array([r[2] for r in rows], F32), np.array([r[3] for r in rows], F32),
            np.array([r[4] for r in rows], F32), np.array([r[5] for r in rows], bool))


# ------------------------------------------------------------------------------------------------
# density grid update
# ------------------------------------------------------------------------------------------------
UPDATE_VARIANTS = ('definition', 'ema below zero', 'no decay', 'mean without clamp', 'ge packbits')
BLOCK = 8192                                             # cells per block of the streaming pass (k_density_apply_mean)
UPDATE_CELLS = (8, 4096, BLOCK, BLOCK + 8, 4 * BLOCK, 257 * BLOCK + 8)   # minimum, H = 16, one block, 8 cells in a 2nd, 4 blocks, > 256 blocks
UPDATE_KINDS = ('dyadic', 'generic')
SCATTER_THREADS = 256
DUP_GROUPS = (2, 3, 64, 1000)
OOB = 8                                                  # indices n_cells .. n_cells + 7; the scratch buffer has that many spare floats
SENTINEL = 123.25
DYADIC_THRESH = 8.0


def fmax_hw(a, b):
    """fp32 max as v_max_f32 computes it (IEEE 754-2019 maximumNumber): -0 < +0, a NaN operand loses"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    out = np.fmax(a, b)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a) & np.signbit(b), F32(-0.0), F32(0.0)), out).astype(F32)


def apply_fresh(g, f, decay, variant='definition'):
    """one cell: grid value g, fresh value f (already scaled) -> new grid value.  renderer.py:517-518: `valid = (grid >= 0) & (tmp >= 0)`,
    `grid[valid] = max(grid[valid] * decay, tmp[valid])`.  -0.0 >= 0 holds; NaN >= 0 and negative >= 0 do not: such a cell keeps g."""
    g, f = np.asarray(g, F32), np.asarray(f, F32)
    with np.errstate(invalid='ignore'):
        ok = (f >= 0) if variant == 'ema below zero' else (f >= 0) & (g >= 0)
        decayed = g if variant == 'no decay' else (g * F32(decay)).astype(F32)
        return np.where(ok, fmax_hw(decayed, f), g).astype(F32)


def mean_of(grid, variant='definition'):
    """float32(exact sum of max(g, 0) / n_cells) -- math.fsum is the correctly rounded sum"""
    g = np.asarray(grid, np.float64)
    if variant != 'mean without clamp':
        g = np.maximum(g, 0.0)
    return F32(math.fsum(g.tolist()) / g.size)


def packbits_model(grid, thresh, cap=None, ge=False):
    """bit i of byte n = grid[8 n + i] > fminf(thresh, cap) (fminf returns the other operand for a NaN); `ge`: the wrong `>=`"""
    t = F32(thresh)
    if cap is not None and not np.isnan(cap):
        t = min(t, F32(cap))
    g = np.asarray(grid).reshape(-1, 8)
    with np.errstate(invalid='ignore'):
        on = (g >= g.dtype.type(t)) if ge else (g > g.dtype.type(t))
    return np.packbits(on, axis=1, bitorder='little').reshape(-1)


def density_update_model(grid, scratch_is_minus_one, sigmas, cells, scale, decay, thresh, variant='definition'):
    """ngp_density_grid_update on a state whose scratch holds -1 everywhere -> dict:
        grid        the grid after an update in which the FIRST sample of a cell wins
        admissible  {cell: set of int32 bit patterns} for every cell sampled more than once: apply_fresh(g, f_k) for each of its samples
        sampled     the distinct cells < n_cells among `cells`
        mean, bitfield   of `grid` (mean_of; packbits against min(thresh, mean))"""
    assert scratch_is_minus_one
    g0 = np.array(grid, F32)
    n_cells = g0.size
    cells = np.asarray(cells, np.int64)
    assert (cells >= 0).all()
    f = (np.asarray(sigmas, F32) * F32(scale)).astype(F32)
    inside = cells < n_cells                                 # an index >= n_cells is ignored
    c, f = cells[inside], f[inside]
    uc, first, counts = np.unique(c, return_index=True, return_counts=True)
    new = g0.copy()
    new[uc] = apply_fresh(g0[uc], f[first], decay, variant)
    admissible = {}
    order = np.argsort(c, kind='stable')
    starts = np.concatenate([[0], np.cumsum(counts)])
    for k in np.nonzero(counts > 1)[0]:
        fk = f[order[starts[k]:starts[k + 1]]]
        admissible[int(uc[k])] = set(_bits(apply_fresh(np.full(len(fk), g0[uc[k]], F32), fk, decay, variant)).tolist())
    mean = mean_of(new, variant)
    return dict(grid=new, admissible=admissible, sampled=uc, mean=mean,
                bitfield=packbits_model(new, thresh, float(mean), ge=variant == 'ge packbits'))


# values of the 'generic' tables: few distinct levels (times factors that are no powers of two), so that no cell comes within 4 ulp of the
# mean or of the threshold by accident -- test_occupancy_cases checks that it does not
_LEVELS = np.array([0.1 * k for k in range(1, 40)], np.float64)
SPECIALS = ('nan', 'negative', 'minus zero on zero', 'equal to decayed', 'minus zero on minus zero')


def update_params(kind, n_cells):
    """-> scale, decay, thresh (fp32-representable floats)"""
    if kind == 'dyadic':
        # every product exact; the threshold (which 2 % of the fresh values equal exactly) decides in half of the tables, the mean (thresh
        # above every value) in the others
        return 0.5, 0.5, DYADIC_THRESH if UPDATE_CELLS.index(n_cells) % 2 == 0 else 64.0
    # the threshold decides in half of the generic tables, the mean (thresh far above it) in the others
    return float(F32(1.7)), float(F32(0.95)), float(F32(0.01)) if UPDATE_CELLS.index(n_cells) % 2 == 0 else 1e9


def _values(rng, kind, n):
    if kind == 'dyadic':
        return (rng.integers(1, 1 << 16, size=n) / 1024.0).astype(F32)      # multiples of 2^-10 below 64
    return (rng.choice(_LEVELS, size=n) * rng.choice([1.0, 3.3, 0.07], size=n)).astype(F32)


def _special_cells(n_cells):
    """cells 5, 6, 1, 7, 2: the initial grid holds ordinary values at 5..7, +0 at 1 and -0 at 2"""
    return dict(zip(SPECIALS, (5, 6, 1, 7, 2)))


@functools.lru_cache(maxsize=None)
def update_table(kind, n_cells):
    """-> dict: grid0 [n_cells] fp32, scale, decay, thresh, calls: list of (sigmas fp32 [n], cells int64 [n]), groups: {copies: cell} of
    calls[1].
      grid0    15 % cells < 0 (-1 and -0.5), 5 % +0, 5 % -0.0, tiny and large values, ordinary ones; cells 0..7 are [-1, +0, -0, tiny, large,
               ordinary x 3]
      call 0   every cell exactly once (a permutation), with the SPECIALS as fresh values of five cells and OOB indices in the middle
      call 1   duplicate groups of 2, 3, 64 and 1000 copies (all values different; one NaN and one negative among the 1000), single
               samples, a NaN and a negative single, OOB indices -- shuffled, so that every group straddles the scatter's blocks
      call 2   n = 0
      call 3   a few single samples; in the generic tables one of them +inf (the mean is +inf from then on)"""
    rng = np.random.default_rng(UPDATE_CELLS.index(n_cells) * 2 + UPDATE_KINDS.index(kind) + 40)
    scale, decay, thresh = update_params(kind, n_cells)
    dyadic = kind == 'dyadic'
    tiny, large = (F32(2.0 ** -10), F32(64 - 2.0 ** -10)) if dyadic else (F32(1e-40), F32(1e6))
    grid = _values(rng, kind, n_cells)
    u = rng.random(n_cells)
    grid[u < 0.10] = -1.0
    grid[(u >= 0.10) & (u < 0.15)] = -0.5
    grid[(u >= 0.15) & (u < 0.20)] = 0.0
    grid[(u >= 0.20) & (u < 0.25)] = -0.0
    grid[(u >= 0.25) & (u < 0.26)] = tiny
    if not dyadic:
        grid[(u >= 0.26) & (u < 0.265)] = F32(1.2e-38)
    grid[rng.integers(0, n_cells, size=3)] = large
    head = _values(rng, kind, 8)
    head[:5] = [-1.0, 0.0, -0.0, tiny, large]
    grid[:8] = head
    special = _special_cells(n_cells)

    def sig(n):
        """fresh sigmas whose product with `scale` is of the table's kind"""
        if not dyadic:
            return _values(rng, kind, n)
        s = (_values(rng, kind, n).astype(np.float64) / scale).astype(F32)
        s[rng.random(n) < 0.02] = DYADIC_THRESH / scale
        return s

    oob = np.arange(n_cells, n_cells + OOB, dtype=np.int64)
    # call 0
    cells0 = rng.permutation(n_cells).astype(np.int64)
    sig0 = sig(n_cells)
    sig0[rng.random(n_cells) < 0.02] = 0.0
    fresh = {'nan': np.nan, 'negative': -3.0, 'minus zero on zero': -0.0, 'minus zero on minus zero': -0.0}
    where0 = np.argsort(cells0)                              # where0[cell] = position of the cell in the permutation
    for name, value in fresh.items():
        sig0[where0[special[name]]] = value
    cell = special['equal to decayed']
    want = F32(grid[cell] * F32(decay))                      # a sigma whose scaled value equals g * decay exactly
    s = F32(np.float64(want) / scale)
    for cand in (s, np.nextafter(s, F32(0)), np.nextafter(s, F32(np.inf))):
        if F32(cand * F32(scale)) == want:
            sig0[where0[cell]] = cand
            break
    else:                                                    # no such sigma: move the cell instead (the products with decay < 1 hit every value)
        f = F32(sig0[where0[cell]] * F32(scale))
        g = F32(np.float64(f) / decay)
        for cand in (g, np.nextafter(g, F32(0)), np.nextafter(g, F32(np.inf))):
            if F32(cand * F32(decay)) == f:
                grid[cell] = cand
                break
        else:
            raise AssertionError('no grid value whose decayed value equals the fresh one')
    half = n_cells // 2
    cells0 = np.concatenate([cells0[:half], oob, cells0[half:]])
    sig0 = np.concatenate([sig0[:half], sig(OOB), sig0[half:]])
    # call 1
    group_cells = rng.choice(n_cells, size=len(DUP_GROUPS), replace=False) if n_cells > 8 else np.array([0, 1, 3, 4])
    n_single = min(n_cells - len(DUP_GROUPS), 3000) if n_cells > 8 else 4
    rest = np.setdiff1d(np.arange(n_cells), group_cells)
    singles = rng.choice(rest, size=n_single, replace=False)
    c1 = [np.full(k, c, np.int64) for k, c in zip(DUP_GROUPS, group_cells)] + [singles.astype(np.int64), oob]
    s1 = [sig(k) + (np.arange(k) * (2.0 ** -9 if dyadic else 0.013)).astype(F32) for k in DUP_GROUPS] + [sig(n_single), sig(OOB)]
    s1[3][17], s1[3][600] = np.nan, -2.0
    s1[4][0], s1[4][1] = np.nan, -0.25
    cells1, sig1 = np.concatenate(c1), np.concatenate(s1).astype(F32)
    perm = rng.permutation(len(cells1))
    cells1, sig1 = cells1[perm], sig1[perm]
    for c in group_cells:                                    # a group that the shuffle left inside one block: move one copy a block on
        pos = np.nonzero(cells1 == c)[0]
        if len(set((pos // SCATTER_THREADS).tolist())) < 2:
            a, b = pos[0], (pos[0] + SCATTER_THREADS) % len(cells1)
            cells1[[a, b]], sig1[[a, b]] = cells1[[b, a]], sig1[[b, a]]
    # call 3
    n3 = min(n_cells, 5)
    cells3 = np.concatenate([rng.choice(n_cells, size=n3, replace=False).astype(np.int64), oob[:2]])
    sig3 = sig(n3 + 2)
    if not dyadic:
        sig3[1] = np.inf
    calls = [(sig0, cells0), (sig1, cells1), (np.zeros(0, F32), np.zeros(0, np.int64)), (sig3, cells3)]
    return dict(grid0=grid, scale=scale, decay=decay, thresh=thresh, calls=calls, groups=dict(zip(DUP_GROUPS, group_cells.tolist())),
                special=special)


@functools.lru_cache(maxsize=None)
def update_reference(kind, n_cells, variant='definition'):
    """the model through the table's calls, the first duplicate winning -> list of density_update_model results"""
    t = update_table(kind, n_cells)
    grid, out = t['grid0'], []
    for sigmas, cells in t['calls']:
        out.append(density_update_model(grid, True, sigmas, cells, t['scale'], t['decay'], t['thresh'], variant))
        grid = out[-1]['grid']
    return out


def ulps_apart(a, b):
    """distance in fp32 steps between two non-negative floats (0 for equal infinities)"""
    return abs(int(_bits(F32(a)).reshape(-1)[0]) - int(_bits(F32(b)).reshape(-1)[0]))


def cells_near(grid, t, ulps=4):
    """how many cells lie within `ulps` fp32 steps of the positive threshold t (the cell equal to it included)"""
    t = F32(t)
    if not np.isfinite(t) or t <= 0:
        return int((np.asarray(grid) == t).sum())
    g = np.asarray(grid, F32)
    pos = g[g > 0]
    return int((np.abs(_bits(pos).astype(np.int64) - int(_bits(t).reshape(-1)[0])) <= ulps).sum())


# every deliberately wrong model, by kernel family (tests/test_occupancy_cases.py shows that the tables tell each from its model)
VARIANTS = dict(coarse=COARSE_VARIANTS[1:], cull=CULL_VARIANTS[1:], update=UPDATE_VARIANTS[1:])


# ------------------------------------------------------------------------------------------------
# packbits
# ------------------------------------------------------------------------------------------------
PACK_SIZES = (1, 255, 256, 257)                           # output bytes


@functools.lru_cache(maxsize=None)
def packbits_cases():
    """-> list of dict(name, grid fp32 [8 N], thresh, cap (None: no cap; may be NaN)): values equal to the effective threshold, one fp32 ulp on
    either side of it (and of the other of thresh / cap), NaN, +-0, +-inf, in every bit position"""
    up, down = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))
    T = F32(0.3)
    out = []
    for N in PACK_SIZES:
        for thresh, cap, what in ((T, None, 'no cap'), (F32(0.0), None, 'threshold 0'), (T, F32(0.5) * T, 'cap below'), (T, T, 'cap equal'),
                                  (T, F32(2.0) * T, 'cap above'), (T, F32(np.nan), 'NaN cap'), (F32(0.0), F32(1.0), 'threshold 0, cap above')):
            pool = [thresh, up(thresh), down(thresh), F32(np.nan), F32(0.0), F32(-0.0), F32(np.inf), F32(-np.inf), F32(1e-45), F32(-1e-45), F32(7.0)]
            if cap is not None and not np.isnan(cap):
                pool += [cap, up(cap), down(cap)]
            pool = np.array(pool, F32)
            idx = (np.arange(N)[:, None] * 3 + np.arange(8)[None, :] * 5) % len(pool)      # 5 and 3 are coprime to 11 and 14
            out.append(dict(name=f'N={N}, {what}', grid=pool[idx].reshape(-1), thresh=float(thresh), cap=None if cap is None else float(cap)))
    return out


@functools.lru_cache(maxsize=None)
def packbits_f64_case():
    """-> grid float64 [8 * 257], thresh: values that exceed the threshold as doubles but equal it once rounded to fp32 (the fp64 kernel
    compares in double: set), the threshold itself, one double step below it, NaN, +-0"""
    T = np.float64(F32(0.3))
    pool = np.array([T, np.nextafter(T, np.inf), T + 1e-12, np.nextafter(T, -np.inf), np.nan, 0.0, -0.0, T * (1 + 2.0 ** -30), 1.0, -1.0, np.inf], np.float64)
    idx = (np.arange(257)[:, None] * 3 + np.arange(8)[None, :] * 5) % len(pool)
    return pool[idx].reshape(-1), float(T)
