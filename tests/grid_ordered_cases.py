"""Tables, inputs and the numpy model of the ordered scatter (csrc/grid_ordered.hip), shared by
tests/test_grid_ordered_cases.py (CPU), tests/test_gpu_grid_ordered.py and tools/bench_grid_ordered.py.  numpy + oracle only.

The model restates THE ORDER of the additions:
  * one record per (point, corner) of a level, slot = b << D | k, key = the entry inside the level (a point outside [0,1]^D: no entry),
    sorted by key, stable;
  * the sorted array is cut into tiles of 64 records.  A fragment (a tile's records of one entry) is summed left to right in fp32, starting
    from its first contribution.  A run that lies inside one tile is added to its entry once, dst = T(float32(dst) + sum);
  * a fragment whose run goes on across the tile's left (right) edge becomes the record (entry, partial sum) at slot 2t (2t + 1) of the next
    array; a fragment that crosses both edges takes slot 2t, and slot 2t + 1 repeats its entry without a value; other slots are empty.
    The same step runs on that array, until an array fits one tile.
`contributions` gives the per-record terms in float64 as the project's float64 oracle does (oracle.grid_backward): positions, fractions,
phi, 1 - phi and phi' are the fp32 values locate() forms from the fp32 inputs, every product and sum after them is float64: w_k g for the
first order, a_k g for the second.

Lattice cases: every point sits at the centre of a cell of ONE level of a table whose scales are 2^l H - 1 (every fraction 1/2: every
weight 2^-D, phi' = 1 or 3/2), so that every contribution of that level is exactly representable in fp32 -- first order: fp32 gradients
with full mantissas; second order: u = few-bit integers times a power of two and gradients that hold fp16 values.  The kernels' fp32
contributions are then the model's, and the bits of that level's entries are the model's bits."""
import functools

import numpy as np

import oracle

TILE = 64
NONE = -1

# small tables, per_level_scale 2 (few-bit scales).  `level`: the level the lattice inputs are made for
TABLES = dict(
    A3=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9), C=2, level=2),   # hashed level
    A3d=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9), C=4, level=0),  # dense level
    A2=dict(cfg=dict(input_dim=2, num_levels=3, per_level_scale=2.0, base_resolution=8, log2_hashmap_size=8), C=4, level=1),
    A4=dict(cfg=dict(input_dim=4, num_levels=2, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=10), C=1, level=1),
    A5=dict(cfg=dict(input_dim=5, num_levels=2, per_level_scale=2.0, base_resolution=2, log2_hashmap_size=10), C=8, level=1),
    TILED=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9), C=2, level=1, gridtype=1),
    ALIGN=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9), C=1, level=2, align=True),
    SMOOTH=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9), C=2, level=1, interp=1),
    # a hashed level of 2^17 entries: three 8-bit digits in the record sort (A3d's level 0 has one, the 2^9 / 2^10 tables two)
    A3h=dict(cfg=dict(input_dim=3, num_levels=3, per_level_scale=2.0, base_resolution=32, log2_hashmap_size=17), C=2, level=2),
)
B_LATTICE = 1000
B_ONE_CELL = 4133     # runs of 4133 records: more than 64 tiles, so at least two further arrays of partial sums


@functools.lru_cache(maxsize=None)
def table(name):
    t = TABLES[name]
    cfg = t['cfg']
    align = t.get('align', False)
    offs, pls = oracle.grid_offsets(align_corners=align, level_dim=t['C'], **cfg)
    offs.setflags(write=False)
    return dict(name=name, offs=offs, S=float(np.log2(pls)), H=cfg['base_resolution'], D=cfg['input_dim'], L=cfg['num_levels'], C=t['C'],
                level=t['level'], gridtype=t.get('gridtype', 0), align=align, interp=t.get('interp', 0))


def general_table(D, C, gridtype=0, align=False, interp=0):
    """the table of the general-input cases: 3 levels, 4 -> x 1.7, 2^9 entries at most (dense and hashed / wrapping levels)"""
    offs, pls = oracle.grid_offsets(input_dim=D, num_levels=3, level_dim=C, per_level_scale=1.7, base_resolution=4, log2_hashmap_size=9,
                                    align_corners=align)
    return dict(name=f'G{D}x{C}', offs=offs, S=float(np.log2(pls)), H=4, D=D, L=3, C=C, level=None, gridtype=gridtype, align=align, interp=interp)


def level_scale(tab, level):
    return float(oracle.grid_level_table(tab['L'], tab['S'], tab['H'])[0][level])


# ---------------------------------------------------------------------------------------------------------------------
# records and their exact contributions
# ---------------------------------------------------------------------------------------------------------------------
def level_position(x, scale, align):
    """(cell, fraction) per point and dimension as locate() forms them: fma(x, scale, 0.5 or 0) rounded once to fp32, floor, the fp32
    difference (exact); and the points inside [0,1]^D"""
    x = np.asarray(x, np.float32)
    pos = (x.astype(np.float64) * float(np.float32(scale)) + (0.0 if align else 0.5)).astype(np.float32)   # (exact in float64, one rounding)
    cell = np.floor(pos)
    frac = (pos - cell).astype(np.float64)
    inside = ((x >= 0) & (x <= 1)).all(axis=1)
    return cell, frac, inside


def record_keys(tab, x, level):
    """[B << D] int64: the entry inside `level` of every record, slot order; NONE for a point outside"""
    idx = oracle.grid_corner_indices(x, tab['offs'], tab['S'], tab['H'], tab['gridtype'], tab['align'])[level].astype(np.int64)
    idx[idx == 0xFFFFFFFF] = NONE
    return idx.reshape(-1)


def contributions(tab, x, g, level, order=1, u=None):
    """[B << D, C] float64, slot order: w_k g[level, b] (order 1) or a_k g[level, b] with a_k = s sum_d u_d sgn_kd phi'_d prod_{m != d} phi_km
    (order 2); zero for points outside"""
    D, C = tab['D'], tab['C']
    scale = level_scale(tab, level)
    _, f, inside = level_position(x, scale, tab['align'])
    # phi, 1 - phi and phi' are the kernels' fp32 values (grid_index.h: locate / locate_d2, every operation rounded to fp32 in their order);
    # everything after them is exact here
    p, one, two, three, six = f.astype(np.float32), np.float32(1), np.float32(2), np.float32(3), np.float32(6)
    if tab['interp'] == 1:
        d1 = (six * p) * (one - p)
        phi = (p * p) * (three - two * p)
    else:
        phi, d1 = p, np.ones_like(p)
    lower = (one - phi).astype(np.float64)
    phi, d1 = phi.astype(np.float64), d1.astype(np.float64)
    B = x.shape[0]
    coef = np.zeros((B, 1 << D), np.float64)
    for k in range(1 << D):
        fk = np.stack([phi[:, d] if (k >> d) & 1 else lower[:, d] for d in range(D)], 1)
        if order == 1:
            coef[:, k] = np.prod(fk, axis=1)
        else:
            a = np.zeros(B)
            for d in range(D):
                sgn = 1.0 if (k >> d) & 1 else -1.0
                a += np.asarray(u, np.float64)[:, d] * sgn * d1[:, d] * np.prod(np.delete(fk, d, axis=1), axis=1)
            coef[:, k] = a * scale
    coef[~inside] = 0.0
    c = coef[:, :, None] * np.asarray(g, np.float64)[level][:, None, :]
    return c.reshape(B << D, C)


def fits_fp32(c):
    return bool(np.array_equal(c.astype(np.float32).astype(np.float64), c))


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def sorted_records(keys, contrib):
    order = np.argsort(keys == NONE, kind='stable')            # records without an entry last ...
    order = order[np.argsort(np.where(keys == NONE, np.iinfo(np.int64).max, keys)[order], kind='stable')]   # ... and a stable sort on the entry
    return keys[order], contrib[order]


def _sum_pass(keys, vals, absent, dst, dtype):
    """one array -> the next (None when this one fits a tile); adds the finished runs into dst"""
    m, C = len(keys), vals.shape[1]
    tiles = -(-m // TILE)
    nk = np.full(2 * tiles, NONE, np.int64)
    nv = np.zeros((2 * tiles, C), np.float32)
    na = np.zeros(2 * tiles, bool)
    for t in range(tiles):
        lo, hi = t * TILE, min(m, t * TILE + TILE)
        i = lo
        while i < hi:
            e = keys[i]
            if e == NONE:
                i += 1
                continue
            j = i + 1
            while j < hi and keys[j] == e:
                j += 1
            rows = vals[i:j][~absent[i:j]]
            acc = np.cumsum(rows, axis=0, dtype=np.float32)[-1]          # left to right in fp32, starting from the first
            left = i == lo and t > 0 and keys[lo - 1] == e
            right = j == lo + TILE and hi < m and keys[hi] == e
            if left:
                nk[2 * t], nv[2 * t] = e, acc
                if right:
                    nk[2 * t + 1], na[2 * t + 1] = e, True
            elif right:
                nk[2 * t + 1], nv[2 * t + 1] = e, acc
            else:
                dst[e] = (dst[e].astype(np.float32) + acc).astype(dtype)
            i = j
    return (nk, nv, na) if tiles > 1 else None


def ordered_sum(keys, contrib, level_size, C, dtype=np.float32, dst=None):
    """the level's table gradient [level_size, C] of dtype `dtype` from its records (slot order), in the documented order; also the number of
    arrays the sum went through"""
    dst = np.zeros((level_size, C), dtype) if dst is None else dst
    k, v = sorted_records(np.asarray(keys, np.int64), np.asarray(contrib, np.float64))
    state = (k, v.astype(np.float32), np.zeros(len(k), bool))
    arrays = 0
    while state is not None:
        arrays += 1
        state = _sum_pass(*state, dst, dtype)
    return dst, arrays


def reversed_sum(keys, contrib, level_size, C):
    """per entry: the same fp32 contributions added one after the other in REVERSE slot order (what another order of the same terms gives)"""
    k, v = sorted_records(np.asarray(keys, np.int64), np.asarray(contrib, np.float64))
    v = v.astype(np.float32)
    out = np.zeros((level_size, C), np.float32)
    n = int((k != NONE).sum())
    starts = np.flatnonzero(np.r_[True, k[1:n] != k[:n - 1]]) if n else np.zeros(0, np.int64)
    for a, b in zip(starts, np.r_[starts[1:], n]):
        out[k[a]] = np.cumsum(v[a:b][::-1], axis=0, dtype=np.float32)[-1]
    return out


def entry_counts(keys, level_size):
    return np.bincount(keys[keys != NONE], minlength=level_size)


def exact_sum(keys, contrib, level_size, C):
    """float64 sums of the contributions and of their magnitudes, per entry"""
    s, a = np.zeros((level_size, C)), np.zeros((level_size, C))
    ok = keys != NONE
    np.add.at(s, keys[ok], contrib[ok])
    np.add.at(a, keys[ok], np.abs(contrib[ok]))
    return s, a


def bound(keys, contrib, level_size, C, D, result=None):
    """the error bound of the general-input cases per entry and channel: (n_e + D + 2) 2^-24 sum|c_i|, n_e the entry's record count: the
    fp32 weight product (D roundings at most), the product with the gradient, n_e - 1 additions and the addition to the entry.  For an fp16
    table (`result` given: the fp16 result as float64) 2^-11 |result| more for the final rounding -- where the result lies below fp16's
    normal range (|result| < 2^-14) the format's spacing is 2^-24 whatever the value, and the term is half of it, 2^-25: no rounding to fp16
    can do better there (2^-11 |result| is the same half spacing, or more, everywhere in the normal range)."""
    _, a = exact_sum(keys, contrib, level_size, C)
    b = (entry_counts(keys, level_size)[:, None] + D + 2) * 2.0 ** -24 * a
    return b if result is None else b + np.maximum(2.0 ** -11 * np.abs(result), 2.0 ** -25)


# ---------------------------------------------------------------------------------------------------------------------
# lattice inputs
# ---------------------------------------------------------------------------------------------------------------------
def centre_coordinates(scale, align):
    """the float32 coordinates in [0, 1] whose position at a level of this scale has the fraction 1/2 exactly (the roundings of x and of the
    fma snap most candidates onto it; the others are left out)"""
    scale = float(np.float32(scale))
    j = np.arange(0, int(np.floor(scale)) + 2)
    x = ((j + (0.5 if align else 0.0)) / scale).astype(np.float32)
    x = x[(x >= 0) & (x <= 1)]
    _, frac, _ = level_position(x[:, None], scale, align)
    return x[frac[:, 0] == 0.5]


@functools.lru_cache(maxsize=None)
def lattice_points(name, B, one_cell=False, seed=0):
    """x [B, D] float32 at cell centres of the table's lattice level: 70 % of the points on 12 centres (long runs), the others anywhere; or all
    of them in ONE cell.  One point outside the unit cube (never with one_cell)."""
    tab = table(name)
    D = tab['D']
    coord = centre_coordinates(level_scale(tab, tab['level']), tab['align'])
    assert len(coord) >= 2
    rng = np.random.default_rng(4100 + seed)
    if one_cell:
        x = np.tile(coord[rng.integers(0, len(coord), D)], (B, 1))
    else:
        hubs = rng.integers(0, len(coord), (12, D))
        pick = np.where(rng.random(B)[:, None] < 0.7, hubs[rng.integers(0, 12, B)], rng.integers(0, len(coord), (B, D)))
        x = coord[pick]
        x[40, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def _spread(rng, shape, span):
    """powers of two 2^-span .. 2^span"""
    return np.exp2(rng.integers(-span, span + 1, shape).astype(np.float64))


@functools.lru_cache(maxsize=None)
def lattice_case(name, order, fp16, one_cell=False, seed=0):
    """dict(tab, x, g [L, B, C] float32, u [B, D] float32 or None, keys, contrib, span).  Gradient magnitudes over 2^-span .. 2^span, span = 12
    narrowed (fp16 tables), and then moved down, until the fp16 gradient and every sum of magnitudes of the lattice level are finite in
    fp16 (then so is every partial sum)."""
    tab = table(name)
    B = B_ONE_CELL if one_cell else B_LATTICE
    x = lattice_points(name, B, one_cell, seed)
    L, D, C, level = tab['L'], tab['D'], tab['C'], tab['level']
    keys = record_keys(tab, x, level)
    size = int(tab['offs'][level + 1] - tab['offs'][level])
    span, shift = 12, 0
    while True:
        rng = np.random.default_rng(4200 + seed + 10 * order + 100 * int(fp16))
        if order == 1 and not fp16:
            g = (rng.uniform(1.0, 2.0, (L, B, C)) * rng.choice([-1.0, 1.0], (L, B, C))).astype(np.float32)   # full mantissas
        else:
            g = oracle.round_fp16(rng.uniform(1.0, 2.0, (L, B, C)) * rng.choice([-1.0, 1.0], (L, B, C)))       # fp16 values
        g = (g * _spread(rng, (L, B, 1), span) * 2.0 ** shift).astype(np.float32)
        u = None
        if order == 2:
            # few-bit integers times one power of two per point: sum_d +-u_d has at most 4 bits
            u = (rng.integers(1, 4, (B, D)) * rng.choice([-1, 1], (B, D)) * _spread(rng, (B, 1), 1 if fp16 else 6)).astype(np.float32)
        contrib = contributions(tab, x, g, level, order, u)
        if not fp16:
            break
        _, a = exact_sum(keys, contrib, size, C)
        if np.abs(g).max() < 6e4 and a.max() < 6e4:
            break
        if span > 0:
            span -= 2
        else:
            shift -= 2   # (the one-cell batch: thousands of terms in one entry)
        assert shift >= -10
    for arr in (g, u, keys, contrib):
        if arr is not None:
            arr.setflags(write=False)
    return dict(tab=tab, x=x, g=g, u=u, keys=keys, contrib=contrib, span=span, shift=shift, level=level, size=size)


LATTICE_NAMES = tuple(TABLES)
