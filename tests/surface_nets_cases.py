"""Numpy models and fields shared by tests/test_surface_nets_cases.py (CPU) and tests/test_gpu_surface_nets.py, test_gpu_lattice_points.py,
test_gpu_extract_mesh.py (GPU): what include/ngp_hip.h states for ngp_surface_nets_count / _emit and ngp_lattice_points.

`surface_nets`      the definition, statement by statement, vectorised: the sign s = f - level (or level - f) in fp32 -- the topology is decided
                    by it and is exact --, one vertex per sign-changing cell numbered in linear cell order, one quad per interior sign-changing
                    lattice edge ordered by (linear index of p) * 3 + axis.  Positions in float64 from the fp32 signs (t = s_a / (s_a - s_b) and
                    the mean without rounding): the kernel's fp32 arithmetic is compared with a tolerance derived from its operations.
`lattice_points`    ngp_lattice_points in fp32, operation by operation (the fused multiply-adds through `fma32`): compared bit for bit.
`is_closed`, `euler`, `signed_volume`, `boundary_edges`   properties of an indexed triangle mesh.
Fields: `sphere`, `torus`, `noise`, `plane_on_lattice`, `noise_with_specials`.  All deterministic; treat the cached ones as read-only."""
import functools

import numpy as np

F32 = np.float32

# the CPU experiment these tests restate: a 40^3 sphere of radius 12.3 lattice units and a torus (R = 11, r = 4), centred off the lattice so
# that no lattice point sits on the level
SPHERE_SHAPE, SPHERE_RADIUS, SPHERE_CENTRE = (40, 40, 40), 12.3, (19.37, 19.61, 19.43)
TORUS_SHAPE, TORUS_R, TORUS_r, TORUS_CENTRE = (24, 40, 40), 11.0, 4.0, (19.37, 19.61, 11.43)


def _signed(volume, level, inside_below):
    f = np.ascontiguousarray(volume, F32)
    assert f.ndim == 3 and min(f.shape) >= 2
    with np.errstate(all='ignore'):
        return (F32(level) - f) if inside_below else (f - F32(level))


def surface_nets(volume, level, inside_below=False, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """volume [nz,ny,nx] -> vertices [V,3] float64 (x, y, z), faces [F,3] int32"""
    s = _signed(volume, level, inside_below)
    nz, ny, nx = s.shape
    inside = s > 0                                   # NaN and s == 0: outside
    s64 = s.astype(np.float64)

    def corner(a, c):                                # corner c = dx + 2 dy + 4 dz of every cell
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    ins = [corner(inside, c) for c in range(8)]
    n_in = np.sum(ins, axis=0)
    active = (n_in > 0) & (n_in < 8)
    cell_id = np.full(active.shape, -1, np.int64)
    cell_id[active] = np.arange(int(active.sum()))   # C order: (k (ny - 1) + j) (nx - 1) + i

    # vertices: the mean of the crossing points, x-edges then y-edges then z-edges, the lower of the two other axes fastest
    total = np.zeros((3,) + active.shape)
    count = np.zeros(active.shape)
    for axis in range(3):
        others = sorted({0, 1, 2} - {axis})
        for e in range(4):
            a = (e & 1) << others[0] | (e >> 1) << others[1]
            b = a + (1 << axis)
            cross = ins[a] != ins[b]
            sa, sb = corner(s64, a), corner(s64, b)
            with np.errstate(all='ignore'):
                t = sa / (sa - sb)
            t = np.clip(np.where(np.isfinite(t), t, 0.5), 0.0, 1.0)
            for d in range(3):
                total[d] += np.where(cross, t if d == axis else float((a >> d) & 1), 0.0)
            count += cross
    kk, jj, ii = np.nonzero(active)
    mean = total[:, kk, jj, ii] / count[kk, jj, ii]
    lattice = mean + np.stack([ii, jj, kk]).astype(np.float64)
    h = np.asarray(spacing, F32).astype(np.float64)
    o = np.asarray(origin, F32).astype(np.float64)
    vertices = (lattice * h[:, None] + o[:, None]).T.copy()

    # faces: the edge p -> p + e_a, interior in b and c, whose ends differ
    cross = np.zeros((nz, ny, nx, 3), bool)
    cross[1:nz - 1, 1:ny - 1, 0:nx - 1, 0] = inside[1:nz - 1, 1:ny - 1, 0:nx - 1] != inside[1:nz - 1, 1:ny - 1, 1:nx]
    cross[1:nz - 1, 0:ny - 1, 1:nx - 1, 1] = inside[1:nz - 1, 0:ny - 1, 1:nx - 1] != inside[1:nz - 1, 1:ny, 1:nx - 1]
    cross[0:nz - 1, 1:ny - 1, 1:nx - 1, 2] = inside[0:nz - 1, 1:ny - 1, 1:nx - 1] != inside[1:nz, 1:ny - 1, 1:nx - 1]
    kk, jj, ii, aa = np.nonzero(cross)               # C order: (linear index of p) * 3 + a
    unit = np.eye(3, dtype=np.int64)
    p = np.stack([ii, jj, kk], axis=1)
    eb, ec = unit[(aa + 1) % 3], unit[(aa + 2) % 3]

    def vertex_of(q):
        ids = cell_id[q[:, 2], q[:, 1], q[:, 0]]
        assert (ids >= 0).all()
        return ids

    q0, q1, q2, q3 = vertex_of(p - eb - ec), vertex_of(p - ec), vertex_of(p), vertex_of(p - eb)
    p_in = inside[kk, jj, ii]
    first = np.stack([q0, np.where(p_in, q1, q3), q2], axis=1)
    second = np.stack([q0, q2, np.where(p_in, q3, q1)], axis=1)
    faces = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, faces


def position_tolerance(shape, origin, spacing):
    """[3] the bound on |kernel - model| per axis, from the kernel's arithmetic with u = 2^-24 (fp32 round to nearest):
      t = s_a / (s_a - s_b): one subtraction, one division, |t| <= 1                              -> 2 u (+ O(u^2))
      the sum of n <= 12 terms in [0, 1]: the k-th partial sum is <= k, its addition errs <= k u    -> (n (n + 1) / 2) u on the sum
      the division by n: the mean is <= 1                                                          -> ((n + 1) / 2 + 2 + 1) u <= 9.5 u on the mean
      + the integer cell coordinate, the result below N                                            -> N u
      fma(lattice, h, o), one rounding of a result of magnitude <= N h + |o|                        -> (N h + |o|) u, and h times what came before
    total <= u (h (9.5 + N) + N h + |o|) <= u (2 N h + 10 h + |o|): a few ulps of max(N h, |o|)."""
    n = np.array(shape[::-1], np.float64)
    h, o = np.abs(np.asarray(spacing, F32).astype(np.float64)), np.abs(np.asarray(origin, F32).astype(np.float64))
    return 2.0 ** -24 * (2.0 * n * h + 10.0 * h + o)


# ------------------------------------------------------------------------------------------------
# mesh properties
# ------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def _edge_keys(e):
    return np.sort(e[:, 0] * (1 << 32) + e[:, 1])


def is_closed(faces):
    """the multiset of directed edges equals the multiset of its reverses"""
    e = directed_edges(faces)
    return len(e) > 0 and np.array_equal(_edge_keys(e), _edge_keys(e[:, ::-1]))


def boundary_edges(faces):
    """the directed edges whose reverse is missing [n,2]"""
    e = directed_edges(faces)
    keys, back = e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]
    return e[~np.isin(keys, back)]


def euler(n_vertices, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return n_vertices - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------
# fields ([nz,ny,nx] fp32; inside is ABOVE the level 0 unless said otherwise)
# ------------------------------------------------------------------------------------------------
def _axes(shape):
    nz, ny, nx = shape
    return np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing='ij')


def sphere(shape, radius, centre):
    """radius - |x - centre| (lattice units, centre = (cx, cy, cz))"""
    z, y, x = _axes(shape)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(F32)


def torus(shape, R, r, centre):
    """r - the distance to the circle of radius R around the z axis through centre"""
    z, y, x = _axes(shape)
    ring = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return (r - np.sqrt(ring ** 2 + (z - centre[2]) ** 2)).astype(F32)


def fitted_sphere(shape):
    """a sphere that fits the box with a margin of more than one cell, centred off the lattice; shapes too small for one get a ball around
    the middle that is cut by the box"""
    nz, ny, nx = shape
    centre = ((nx - 1) * 0.5 + 0.13, (ny - 1) * 0.5 - 0.11, (nz - 1) * 0.5 + 0.07)
    return sphere(shape, max(0.31 * (min(shape) - 1), 0.6), centre)


def fitted_torus(shape):
    nz, ny, nx = shape
    centre = ((nx - 1) * 0.5 + 0.13, (ny - 1) * 0.5 - 0.11, (nz - 1) * 0.5 + 0.07)
    R = 0.28 * (min(nx, ny) - 1)
    return torus(shape, R, max(0.4 * R, 0.55), centre)


def noise(shape, seed=0):
    """standard Gaussian noise: at level 0.5 every corner configuration occurs and the surface touches every boundary"""
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def plane_on_lattice(shape):
    """x - (nx // 2): a whole lattice plane has s == 0 exactly (outside), its neighbours differ in sign"""
    z, y, x = _axes(shape)
    return (x - float(shape[2] // 2)).astype(F32)


def noise_with_specials(shape, seed=1):
    """noise with one value in eight replaced by NaN, +inf, -inf or the level 0.5 itself (an exact tie)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(F32)
    pick = rng.integers(0, 32, shape)
    for code, value in enumerate((np.nan, np.inf, -np.inf, 0.5)):
        f[pick == code] = value
    return f


@functools.lru_cache(maxsize=None)
def reference_sphere():
    f = sphere(SPHERE_SHAPE, SPHERE_RADIUS, SPHERE_CENTRE)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference_torus():
    f = torus(TORUS_SHAPE, TORUS_R, TORUS_r, TORUS_CENTRE)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------
# the culled lattice
# ------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) for fp32 arrays: the product of two fp32 values is exact in float64; the float64 sum is turned into a round-to-odd sum
    (TwoSum gives its error exactly), which rounds to fp32 like the exact sum does"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    up = np.nextafter(s, np.inf)
    down = np.nextafter(s, -np.inf)
    s = np.where(even & (err > 0), up, np.where(even & (err < 0), down, s))
    return s.astype(F32)


def lattice_spacing(lo, hi, dims):
    """h = (hi - lo) / (N - 1) in double, narrowed once; o = lo narrowed: what raymarching.lattice_points hands to the kernel"""
    lo, hi, n = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(dims, np.float64)
    return lo.astype(F32), ((hi - lo) / (n - 1)).astype(F32)


def dilate_volumes(vol, dilate):
    """bool [C,z,y,x] -> a cell is set iff a cell of the (2 dilate + 1)^3 box around it, cut at the grid's faces, is set"""
    if dilate == 0:
        return vol
    C, H = vol.shape[0], vol.shape[1]
    pad = np.zeros((C, H + 2 * dilate, H + 2 * dilate, H + 2 * dilate), bool)
    pad[:, dilate:dilate + H, dilate:dilate + H, dilate:dilate + H] = vol
    out = np.zeros_like(vol)
    for dz in range(2 * dilate + 1):
        for dy in range(2 * dilate + 1):
            for dx in range(2 * dilate + 1):
                out |= pad[:, dz:dz + H, dy:dy + H, dx:dx + H]
    return out


def lattice_cells(x, y, z, bound, C, H):
    """fp32 positions -> (cascade, cx, cy, cz): the marcher's position term of the cascade and probe_geom's index statement"""
    bound = F32(bound)
    mx = np.maximum(np.abs(x), np.maximum(np.abs(y), np.abs(z)))
    level = np.clip(np.frexp(mx)[1], 0, C - 1).astype(np.int64)
    pw = np.ldexp(F32(1), level).astype(F32)
    capped = ~(pw < bound)
    rb = np.where(capped, F32(1) / bound, np.ldexp(F32(1), -level).astype(F32)).astype(F32)

    def cell(v):
        c = (F32(0.5) * fma32(v, rb, F32(1))) * F32(H)
        return np.clip(c, F32(0), F32(H - 1)).astype(np.int64)

    return level, cell(x), cell(y), cell(z)


def lattice_points(lo, hi, dims, z0, z1, bits=None, bound=1.0, cascade=1, grid_size=128, dilate=1, dilated=None):
    """-> points [K,3] fp32, index [K] int32, keep [z1 - z0, ny, nx] bool.  dims = (nx, ny, nz); dilated: dilate_volumes(unpack_volumes(bits))
    when the caller has it already"""
    nx, ny, nz = dims
    o, h = lattice_spacing(lo, hi, dims)
    k, j, i = np.meshgrid(np.arange(z0, z1), np.arange(ny), np.arange(nx), indexing='ij')
    x, y, z = fma32(i.astype(F32), h[0], o[0]), fma32(j.astype(F32), h[1], o[1]), fma32(k.astype(F32), h[2], o[2])
    if bits is None and dilated is None:
        keep = np.ones(x.shape, bool)
    else:
        if dilated is None:
            import occupancy_cases as oc
            dilated = dilate_volumes(oc.unpack_volumes(bits, cascade, grid_size), dilate)
        level, cx, cy, cz = lattice_cells(x, y, z, bound, cascade, grid_size)
        keep = dilated[level, cz, cy, cx]
    index = ((k * ny + j) * nx + i).astype(np.int32)
    points = np.stack([x[keep], y[keep], z[keep]], axis=1).astype(F32)
    return points, index[keep], keep
