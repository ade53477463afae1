"""The float64 model of the grid forward and the inputs of tests/test_gpu_grid_forward.py (conditions on those inputs: asserted on the CPU by
tests/test_grid_forward_cases.py).  numpy + oracle only: nothing here touches a GPU.

`grid_reference` restates the forward as the kernels compute it: the oracle's corner indices, fp32 fractions formed expression for
expression as grid_index.h: locate() forms them, float64 products and sums.  tests/test_gpu_fp64.py pins fp64.hip to it; here it pins
k_grid_forward<.., true> (dy_dx), k_grid_forward_pair and the three bodies of k_grid_forward_fast (csrc/gridencoder.hip).

A rounding tolerance hides a misrouted corner or a swapped weight, so the lattice cases have no rounding at all.  The points are those of
tests/grid_lattice_cases.py (S = 0, H - 1 a power of two, fractions multiples of 1 / sub) and the table holds j * 2^-6 with integers
|j| <= jmax drawn independently per entry and channel.  A corner weight is a multiple of 1 / sub^D and the 2^D weights of a point sum to 1,
so every product, every partial sum in any order and the output are integer multiples of unit = 2^-6 / sub^D of magnitude <= jmax * sub^D
units: exact in fp32, and representable in the table type when jmax * sub^D <= 2^11 (fp16) or 2^24 (fp32).  dy_dx: the weights of the
other D - 1 coordinates, times the level scale (a power of two), times phi' (1, or 3/2 at fraction 1/2 under smoothstep), times a
difference of two table values: <= 2 * jmax * sub^(D-1) (* 3) units of scale * 2^-6 / sub^(D-1) (/ 2).  The kernels' outputs must equal
the float64 model bit for bit.

What the lattice cannot show: every level has the same scale (S = 0), and smoothstep maps the fractions 0 and 1/2 to themselves, so on the
lattice it changes dy_dx alone.  A level located with another level's scale, or smoothstep left out of a scheduled kernel, shows in the
off-lattice cases at the end of this module, within a rounding bound.

A case's points come from a POOL: glc.points(base) with base.B = glc.B_SMALL points (the planted corners x = 0 and x = 1, both kinds of
outside point, runs of identical points, a walk).  A run over B points takes the last B points of the pool, or the whole pool followed by
B - pool seeded re-draws from it, so the reference is computed once on the pool and gathered."""
import collections
import functools
import itertools

import numpy as np

import oracle
import grid_lattice_cases as glc


# ---------------------------------------------------------------------------------------------------------------------
# the float64 model
# ---------------------------------------------------------------------------------------------------------------------
def unit_inputs(x, bound=0.0):
    """InputMap of grid_index.h in fp32: (x + bound) * (1 / (2 bound)), two roundings; bound = 0: the inputs are unit coordinates"""
    x = np.asarray(x, np.float32)
    if not bound > 0.0:
        return x
    return ((x + np.float32(bound)).astype(np.float32) * np.float32(1.0 / (2.0 * float(bound)))).astype(np.float32)


def frac32(x, scale, align, interp):
    """fractions and smoothstep derivative exactly as grid_index.h: locate() computes them (fp32, same operation order)"""
    p = (x.astype(np.float64) * np.float64(scale) + (0.0 if align else 0.5)).astype(np.float32)   # fmaf: exact here, one rounding
    f = (p - np.floor(p)).astype(np.float32)
    one = np.float32(1)
    if interp == 1:
        deriv = (np.float32(6) * f) * (one - f)
        f = (f * f) * (np.float32(3) - np.float32(2) * f)
    else:
        deriv = np.ones_like(f)
    return f, deriv


def grid_reference(x, emb, offs, S, H, gridtype, align, interp, bound=0.0, with_dydx=True):
    """fp64 restatement: oracle corner indices, fp32 weights as the kernel forms them, fp64 products and sums.
    -> outputs [L,B,C], dy_dx [B,L,D,C] (None without with_dydx), per level (indices [B,2^D] global, weights [B,2^D] fp32, inside mask),
    and A [L,B,C] = sum_k |w_k * v_k| (what a rounding bound of the output is made from)"""
    x = unit_inputs(x, bound)
    emb = np.asarray(emb, np.float64)
    B, D = x.shape
    C = emb.shape[1]
    L = len(offs) - 1
    idx = oracle.grid_corner_indices(x, offs, S, H, gridtype, align)
    scale, _ = oracle.grid_level_table(L, S, H)
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    out = np.zeros((L, B, C))
    A = np.zeros((L, B, C))
    dydx = np.zeros((B, L, D, C)) if with_dydx else None
    levels = []
    for l in range(L):
        f, deriv = frac32(x, scale[l], align, interp)
        gidx = offs[l] + idx[l].astype(np.int64)
        gidx[~inside] = 0
        ws = np.zeros((B, 1 << D), np.float32)
        for k in range(1 << D):
            w = np.ones(B, np.float32)
            for d in range(D):
                w = w * (f[:, d] if (k >> d) & 1 else np.float32(1) - f[:, d])
            ws[:, k] = w
            term = w.astype(np.float64)[:, None] * emb[gidx[:, k]]
            out[l] += term
            A[l] += np.abs(term)
        for g in range(D if with_dydx else 0):
            for k in range(1 << D):
                if (k >> g) & 1:
                    continue
                w = np.full(B, scale[l], np.float32)
                for d in range(D):
                    if d != g:
                        w = w * (f[:, d] if (k >> d) & 1 else np.float32(1) - f[:, d])
                wd = (w * deriv[:, g]).astype(np.float64)
                dydx[:, l, g] += wd[:, None] * (emb[gidx[:, k | (1 << g)]] - emb[gidx[:, k]])
        out[l][~inside] = 0
        A[l][~inside] = 0
        if with_dydx:
            dydx[~inside, l] = 0
        levels.append((gidx, ws, inside))
    return out, dydx, levels, A


# ---------------------------------------------------------------------------------------------------------------------
# which kernel, which body, which tile size (csrc/gridencoder.hip: launch_forward, k_grid_forward_fast; csrc/grid_index.h: LevelIndexer)
# ---------------------------------------------------------------------------------------------------------------------
Indexer = collections.namedtuple('Indexer', 'stride size mask hashed need_mod')


def level_indexer(D, gridtype, align, size, resolution):
    """LevelIndexer<D>::init (uint32 arithmetic)"""
    s, stride = 1, []
    for _ in range(D):
        if s <= size:
            stride.append(s)
            s = (s * (resolution if align else resolution + 1)) & 0xFFFFFFFF
        else:
            stride.append(0)
    hashed = gridtype == 0 and s > size
    need_mod = hashed or s > size or bool(align)
    mask = size - 1 if size & (size - 1) == 0 else 0
    return Indexer(tuple(stride), size, mask, hashed, need_mod)


def scheduled_kernel(dtype, D, C, align):
    """the kernel launch_forward picks when dy_dx == NULL"""
    return 'fast' if dtype == 'f16' and D == 3 and C == 2 and not align else 'pair'


def level_body(dtype, D, C, gridtype, align, size, resolution):
    """the body a level's workgroups take: `pair` (k_grid_forward_pair), or inside k_grid_forward_fast `dense`, `hashed_pow2` or `generic`"""
    if scheduled_kernel(dtype, D, C, align) == 'pair':
        return 'pair'
    ix = level_indexer(3, gridtype, False, size, resolution)
    if not ix.hashed and not ix.need_mod and ix.stride[0] == 1 and ix.stride[1] != 0 and ix.stride[2] != 0:
        return 'dense'
    if ix.hashed and ix.mask != 0:
        return 'hashed_pow2'
    return 'generic'


def launch_ppb(B, L):
    """points per workgroup of the scheduled launch (launch_forward)"""
    ppb = 1024
    while ppb > 128 and -(-B // ppb) * L < 2048:
        ppb >>= 1
    return ppb


# ---------------------------------------------------------------------------------------------------------------------
# lattice cases
# ---------------------------------------------------------------------------------------------------------------------
FCase = collections.namedtuple('FCase', 'name base Bs jmax bound level_cost')
JMAX = {'f16': 15, 'f32': 1000}
SENTINEL = {'f16': 0x5A5A, 'f32': 0x5A5A5A5A}   # the bit pattern the output buffers are pre-filled with (finite, not a multiple of any unit)


def fcase(name, base, Bs=None, bound=0.0, level_cost=None):
    assert base.B == glc.B_SMALL
    return FCase(name, base, tuple(Bs) if Bs is not None else (base.B,), JMAX[base.dtype], float(bound),
                 None if level_cost is None else tuple(float(c) for c in level_cost))


def case_id(fc):
    tail = '' if fc.Bs == (fc.base.B,) else ('-B' + '+'.join(str(b) for b in fc.Bs) if len(fc.Bs) <= 2 else '-%dBs' % len(fc.Bs))
    sizes = 'x'.join(str(s) for s in fc.base.level_sizes) if len(fc.base.level_sizes) <= 4 else 'L%d' % len(fc.base.level_sizes)
    return '%s-%s-C%d-D%d-%s%s%s-%s%s' % (fc.name, fc.base.dtype, fc.base.C, fc.base.D, 'tiled' if fc.base.gridtype else 'hash',
                                          '-align' if fc.base.align else '', '-smooth' if fc.base.interp else '', sizes, tail)


def out_unit(fc):
    return 2.0 ** -6 / fc.base.sub ** fc.base.D


def dydx_unit(fc):
    return (fc.base.H - 1) * 2.0 ** -6 / fc.base.sub ** (fc.base.D - 1) / (2 if fc.base.interp else 1)


def exact_conditions(fc):
    """(largest |output| and largest |dy_dx| in their units, the cap of the table type): both must stay at or below the cap"""
    b = fc.base
    return fc.jmax * b.sub ** b.D, 2 * fc.jmax * b.sub ** (b.D - 1) * (3 if b.interp else 1), glc.cap_of(b)


@functools.lru_cache(maxsize=None)
def table(fc, which=0):
    """[entries, C] float32: j * 2^-6, |j| <= jmax, independent per entry and channel (which = 1: a second table from another seed)"""
    n = int(sum(fc.base.level_sizes))
    rng = np.random.default_rng(5000 + 97 * fc.base.seed + which)
    t = (rng.integers(-fc.jmax, fc.jmax + 1, (n, fc.base.C)) * 2.0 ** -6).astype(np.float32)
    t.setflags(write=False)
    return t


def point_index(fc, B):
    """which pool points a run over B points takes"""
    P = fc.base.B
    if B <= P:
        return np.arange(P - B, P)
    return np.concatenate([np.arange(P), np.random.default_rng(7000 + B).integers(0, P, B - P)])


def level_bodies(fc):
    b = fc.base
    return [level_body(b.dtype, b.D, b.C, b.gridtype, b.align, s, b.H) for s in b.level_sizes]   # (S = 0: every level's resolution is H)


@functools.lru_cache(maxsize=None)
def reference(fc, which=0):
    """the float64 model on the case's pool, in unit coordinates: dict(x, offs, S, H, out [L,P,C], dydx [P,L,D,C], A, inside, levels)"""
    b = fc.base
    x, offs, S = glc.points(b)
    out, dydx, levels, A = grid_reference(x, table(fc, which), offs, S, b.H, b.gridtype, b.align, b.interp)
    inside = levels[0][2]
    for a in (out, dydx, A, inside):
        a.setflags(write=False)
    return dict(x=x, offs=offs, S=S, H=b.H, out=out, dydx=dydx, A=A, inside=inside, levels=levels)


def inputs(fc):
    """the pool as the call receives it: unit coordinates, or world coordinates for a case with a bound"""
    x = reference(fc)['x']
    if fc.bound > 0.0:
        assert fc.bound == glc.BOUND
        return glc.world_coordinates(x)
    return x


LEVEL_SIZES_3 = lambda align: (1024, glc.dense_size(3, 17, align), 1000, 8)   # hashed | dense | hashed, no power of two | tiny (tiled: wrapping)

# LAYOUT: 2 dtypes x C x D, index modes in rotation, one level -- the cases of the backward tests (every instantiation of
# k_grid_forward_pair and of k_grid_forward<.., true>)
LAYOUT = [fcase('layout', c) for c in glc.LAYOUT_CASES]

# SWEEP: (3, 2), gridtype x align_corners x interpolation over four levels of one scale
SWEEP = [fcase('sweep', glc.make_case(3, 2, dtype, gridtype=gt, align=al, interp=ip, level_sizes=LEVEL_SIZES_3(al), seed=400 + i))
         for dtype in ('f32', 'f16') for i, (gt, al, ip) in enumerate(itertools.product((0, 1), (False, True), (0, 1)))]

# MAPPED: world coordinates at bound = 2
MAPPED = [fcase('mapped', glc.make_case(3, 2, 'f16', level_sizes=LEVEL_SIZES_3(False), seed=420), bound=glc.BOUND),
          fcase('mapped', glc.make_case(3, 2, 'f16', interp=1, level_sizes=LEVEL_SIZES_3(False), seed=421), bound=glc.BOUND),
          fcase('mapped', glc.make_case(3, 2, 'f32', level_sizes=LEVEL_SIZES_3(False), seed=422), bound=glc.BOUND),
          fcase('mapped', glc.make_case(2, 4, 'f16', level_sizes=(1024, glc.dense_size(2, 33, False), 1000, 8), seed=423), bound=glc.BOUND)]


def ladder_sizes(L):
    return tuple(LEVEL_SIZES_3(False)[l % 4] for l in range(L))


# LADDER: 32 levels; per tile size the smallest B that selects it (63 tiles and one point, 1 for the smallest tile) and another B whose last
# tile holds one point; and level counts around the 8 XCD lists at B = 4133
LADDER_BS = ((1, 5 * 128 + 1), 63 * 256 + 1, 70 * 256 + 1, 63 * 512 + 1, 64 * 512 + 1, 63 * 1024 + 1, 64 * 1024 + 1)
LADDER_LS = (1, 7, 8, 9, 17)
LADDER = [fcase('ladder', glc.make_case(3, 2, dtype, level_sizes=ladder_sizes(32), seed=440 + i), Bs=B if isinstance(B, tuple) else (B,))
          for i, dtype in enumerate(('f16', 'f32')) for B in LADDER_BS] + \
         [fcase('ladder', glc.make_case(3, 2, dtype, level_sizes=ladder_sizes(L), seed=450 + 10 * i + L))
          for i, dtype in enumerate(('f16', 'f32')) for L in LADDER_LS]

# TINY: fewer points than a wave, a wave and a workgroup step hold, and one more
TINY_BS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)
TINY = [fcase('tiny', glc.make_case(3, 2, 'f16', level_sizes=(glc.dense_size(3, 17, False),), seed=480), Bs=TINY_BS),
        fcase('tiny', glc.make_case(3, 2, 'f16', level_sizes=(1024,), seed=481), Bs=TINY_BS),
        fcase('tiny', glc.make_case(2, 8, 'f32', level_sizes=(1024,), seed=482), Bs=TINY_BS),
        fcase('tiny', glc.make_case(5, 1, 'f16', level_sizes=(1024,), seed=483), Bs=TINY_BS)]

# COSTS: a skewed level_cost moves tiles of the last level to other XCDs' lists
COSTS = [fcase('costs', glc.make_case(3, 2, dtype, level_sizes=ladder_sizes(32), seed=440 + i), Bs=(70 * 256 + 1,), level_cost=[1.0] * 31 + [40.0])
         for i, dtype in enumerate(('f16', 'f32'))]

ALL = LAYOUT + SWEEP + MAPPED + LADDER + TINY + COSTS


# ---------------------------------------------------------------------------------------------------------------------
# (f) off the lattice, multi-resolution
# ---------------------------------------------------------------------------------------------------------------------
OFF_B, OFF_H, OFF_L = 3001, 16, 8
OFF_MODES = [(0, False, 0), (0, False, 1), (1, False, 0), (1, False, 1), (0, True, 0), (1, True, 1)]   # gridtype, align_corners, interp
# D, C, dtype, gridtype, align_corners, interp, bound, log2_hashmap_size.  At 2^12 every level of a D = 3 table is hashed (17^3 > 4096; the
# coarse levels are dense for D = 2 only), so three more (3, 2, fp16) cases at 2^15 reach the dense body of k_grid_forward_fast off the lattice
OFF_CASES = [(3, 2, dtype, gt, al, ip, 0.0, 12) for dtype in ('f16', 'f32') for gt, al, ip in OFF_MODES] + \
            [(2, 2, 'f16', 0, False, 1, 0.0, 12), (3, 4, 'f32', 1, False, 0, 0.0, 12), (4, 2, 'f16', 0, True, 0, 0.0, 12),
             (5, 1, 'f32', 0, False, 1, 0.0, 12), (3, 8, 'f16', 1, True, 1, 0.0, 12), (3, 2, 'f16', 0, False, 0, 2.0, 12),
             (3, 2, 'f16', 0, False, 0, 0.0, 15), (3, 2, 'f16', 0, False, 1, 0.0, 15), (3, 2, 'f16', 0, False, 1, 2.0, 15)]


def edge_points(B, D, rng):
    """_points() of tests/test_gpu_grid.py: uniform plus the edge rows"""
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0
    x[2] = np.nextafter(np.float32(1.0), np.float32(2.0))  # just outside
    x[3, 0] = -1e-7                                         # just outside
    x[4] = 0.5
    x[5] = np.float32(1.0) - np.float32(2 ** -24)
    x[6, :] = [1.0, 0.0, 0.5][:D] if D <= 3 else [1.0, 0.0, 0.5, 0.25, 0.75][:D]
    return x


@functools.lru_cache(maxsize=None)
def off_lattice_case(D, C, dtype, gridtype, align, interp, bound, log2_size=12):
    """x (world coordinates when bound > 0), table, offsets, S, H and from the float64 model ref, A [L,B,C] and the element-wise bound
        |got - ref| <= A * (2 D + 2^D + 1) * 2^-24 + |ref| * eps_T + floor_T
    one rounding per fraction (fma and subtraction are exact or one rounding; smoothstep's are charged to the 2 D), D - 1 for the weight
    product, one per fma or add (2^D of them and the pair's final add), each of a quantity <= A; the rounding to the table type is relative
    (eps_T = 2^-24 | 2^-11) down to fp16's subnormal spacing (floor_T = 0 | 2^-25)"""
    rng = np.random.default_rng(600 + 10 * D + C + (100 if dtype == 'f16' else 0) + 1000 * gridtype + 2000 * int(align) + 4000 * interp + log2_size)
    offs, pls = oracle.grid_offsets(input_dim=D, num_levels=OFF_L, level_dim=C, per_level_scale=1.3819, base_resolution=OFF_H, log2_hashmap_size=log2_size,
                                    align_corners=align)
    S = float(np.log2(pls))
    emb = rng.uniform(-1, 1, (int(offs[-1]), C)).astype(np.float32)
    if dtype == 'f16':
        emb = oracle.round_fp16(emb)
    x = edge_points(OFF_B, D, rng)
    if bound > 0.0:
        x = (x * np.float32(2.0 * bound) - np.float32(bound)).astype(np.float32)
    ref, _, levels, A = grid_reference(x, emb, offs, S, OFF_H, gridtype, align, interp, bound=bound, with_dydx=False)
    eps, floor = (2.0 ** -11, 2.0 ** -25) if dtype == 'f16' else (2.0 ** -24, 0.0)
    tol = A * (2 * D + 2 ** D + 1) * 2.0 ** -24 + np.abs(ref) * eps + floor
    _, res = oracle.grid_level_table(OFF_L, S, OFF_H)
    bodies = [level_body(dtype, D, C, gridtype, align, int(offs[l + 1] - offs[l]), int(res[l])) for l in range(OFF_L)]
    for a in (x, emb, offs, ref, A, tol):
        a.setflags(write=False)
    return dict(x=x, emb=emb, offs=offs, S=S, H=OFF_H, ref=ref, A=A, tol=tol, inside=levels[0][2], bodies=bodies)
