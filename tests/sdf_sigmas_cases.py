"""Cases and references shared by tests/test_sdf_sigmas_cases.py, tests/test_sdf_sigmas_abi.py (CPU), tests/test_gpu_sdf_sigmas.py and
tests/test_gpu_network_sdf.py (GPU): raymarching.sdf_sigmas, NeuS's section opacity as the density that reproduces it.

`definition` is the op's definition in plain torch at the dtype of its inputs (autograd gives the gradients): in float64 on the CPU it is
THE reference, in float32 on the CPU the yardstick of the fp32 kernels' rounding error, on the GPU the "torch chain" the op replaces.
`literal_alpha` is NeuS's own formula (models/renderer.py), float64.

ONE sample table (`sample_table`): M = 1600 rows, the last 100 padding (d0 = 0, arbitrary finite values elsewhere), evaluated over the grid
INV_S x COS_ANNEAL.  Rows on a relu kink of the cosine (|c| < 1e-3, |c - 1| < 1e-3) or with x within 1e-3 of the cap at any grid point were
redrawn when the table was built: no comparison skips a row.

Error measures: the forward error on x = sigma * d0 (the quantity the compositors see), the gradients as those of sum_i w_i x_i -- the
upstream gradient of sigma_i is UP_i = fp32(w_i d0_i), i.e. the gradients are measured "times d0", grad_inv_s on the same scale.  Padding rows
carry a non-zero upstream gradient too."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS, X_MAX = 1e-5, 15.0
M, LIVE = 1600, 1500
INV_S = (20.0, 64.0, 512.0, 3000.0)
COS_ANNEAL = (0.0, float(np.float32(0.3)), 1.0)     # the C ABI takes cos_anneal as a 32-bit float: float32-representable values
GRID = tuple((s, a) for s in INV_S for a in COS_ANNEAL)
KEYS = ('x', 'grad_sdf', 'grad_normals', 'grad_dirs', 'grad_inv_s')
KINK, CAP_MARGIN = 1e-3, 1e-3


def section_x(sdf, normals, dirs, d0, inv_s, cos_anneal):
    """x = -log(1 - alpha) of NeuS's section opacity, uncapped, in the cancellation-free form; (x, c)"""
    c = (dirs * normals).sum(-1)
    ic = -(F.relu(0.5 - 0.5 * c) * (1.0 - cos_anneal) + F.relu(-c) * cos_anneal)
    h = 0.5 * ic * d0
    return torch.log(torch.sigmoid(inv_s * (sdf - h)) + EPS) - F.logsigmoid(inv_s * (sdf + h)), c   # softplus(-u) = -logsigmoid(u)


def definition(sdf, normals, dirs, deltas, inv_s, cos_anneal=1.0):
    """sigmas [M] of raymarching.sdf_sigmas in plain torch ops (any dtype, any device), differentiable"""
    d0 = deltas[:, 0]
    x, _ = section_x(sdf, normals, dirs, d0, inv_s, cos_anneal)
    live = d0 > 0
    return torch.where(live, torch.clamp(x, max=X_MAX) / torch.where(live, d0, torch.ones_like(d0)), torch.zeros_like(x))


def literal_alpha(sdf, normals, dirs, d0, inv_s, cos_anneal):
    """NeuS: alpha = clip((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5), 0, 1) (float64 tensors)"""
    c = (dirs * normals).sum(-1)
    ic = -(F.relu(0.5 - 0.5 * c) * (1.0 - cos_anneal) + F.relu(-c) * cos_anneal)
    prev = torch.sigmoid((sdf - ic * d0 * 0.5) * inv_s)
    nxt = torch.sigmoid((sdf + ic * d0 * 0.5) * inv_s)
    return ((prev - nxt + EPS) / (prev + EPS)).clip(0.0, 1.0)


def _draw(rng, n):
    sdf = rng.uniform(-0.1, 0.1, n)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    normals = unit(rng.normal(size=(n, 3))) * rng.uniform(0.7, 1.3, (n, 1))
    dirs = unit(rng.normal(size=(n, 3)))
    d0 = rng.uniform(0.005, 0.05, n)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(sdf), f32(normals), f32(dirs), f32(d0)


def _violations(sdf, normals, dirs, d0):
    """rows on a relu kink, or within CAP_MARGIN of the cap at some grid point"""
    t = [torch.from_numpy(a) for a in (sdf, normals, dirs, d0)]
    bad = np.zeros(len(sdf), bool)
    for inv_s, ca in GRID:
        x, c = section_x(*t, torch.tensor(inv_s, dtype=torch.float64), ca)
        bad |= ((x - X_MAX).abs() < CAP_MARGIN).numpy() | (c.abs() < KINK).numpy() | ((c - 1.0).abs() < KINK).numpy()
    return bad


@functools.lru_cache(maxsize=None)
def sample_table():
    """-> dict of float64 numpy arrays with float32-representable values: sdf [M], normals [M,3], dirs [M,3] (unit up to fp32 rounding),
    deltas [M,2] (column 0 = 0 in the padding), up [M] (the upstream gradient of sigma)"""
    rng = np.random.default_rng(20261021)
    sdf, normals, dirs, d0 = _draw(rng, M)
    for _ in range(64):
        bad = _violations(sdf[:LIVE], normals[:LIVE], dirs[:LIVE], d0[:LIVE])
        if not bad.any():
            break
        idx = np.nonzero(bad)[0]
        sdf[idx], normals[idx], dirs[idx], d0[idx] = _draw(rng, len(idx))
    else:
        raise AssertionError('sample_table: the redraw did not converge')
    d1 = rng.uniform(0.005, 0.05, M).astype(np.float32).astype(np.float64)
    d0[LIVE:] = 0.0
    w = rng.uniform(-1.0, 1.0, M)
    up = np.where(d0 > 0, w * d0, w).astype(np.float32).astype(np.float64)
    return dict(sdf=sdf, normals=normals, dirs=dirs, deltas=np.stack([d0, d1], 1), up=up)


def evaluate(inv_s, cos_anneal, dtype, rows=M):
    """`definition` on the first `rows` rows of the table at `dtype` on the CPU, gradients of sum(up * sigma) by autograd -> dict of float64 numpy
    arrays: x = sigma * d0 [rows], sigma, grad_sdf, grad_normals, grad_dirs, grad_inv_s [1]"""
    t = sample_table()
    leaf = lambda a: torch.tensor(a[:rows]).to(dtype).requires_grad_(True)
    sdf, normals, dirs = leaf(t['sdf']), leaf(t['normals']), leaf(t['dirs'])
    deltas, up = torch.tensor(t['deltas'][:rows]).to(dtype), torch.tensor(t['up'][:rows]).to(dtype)
    s = torch.tensor([inv_s], dtype=dtype, requires_grad=True)
    sigma = definition(sdf, normals, dirs, deltas, s, cos_anneal)
    grads = torch.autograd.grad((up * sigma).sum(), (sdf, normals, dirs, s))
    out = {k: g.detach().double().numpy() for k, g in zip(KEYS[1:], grads)}
    out['sigma'] = sigma.detach().double().numpy()
    out['x'] = out['sigma'] * t['deltas'][:rows, 0]
    return out


@functools.lru_cache(maxsize=None)
def reference(inv_s, cos_anneal):
    """the float64 definition on the whole table + `capped` [M] (live rows whose uncapped x is above the cap) and the uncapped `x_raw`"""
    t = sample_table()
    out = evaluate(inv_s, cos_anneal, torch.float64)
    x_raw, _ = section_x(*(torch.from_numpy(t[k]) for k in ('sdf', 'normals', 'dirs')), torch.from_numpy(t['deltas'][:, 0]),
                         torch.tensor(inv_s, dtype=torch.float64), cos_anneal)
    out['x_raw'] = x_raw.numpy()
    out['capped'] = (out['x_raw'] > X_MAX) & (t['deltas'][:, 0] > 0)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(key):
    """bound of the fp32 kernels' error in `key` over the whole grid: 4 x the max error of the same definition evaluated in float32 torch on the
    CPU against float64 (the rounding of the same formulas in the same format; the factor covers the device's exp / log and the operation
    order) + 1e-7 of the largest reference value -- the rule of tests/composite_geo_cases.py.  -> (bound, measured float32 error)"""
    err = ref_max = 0.0
    for inv_s, ca in GRID:
        ref, f32 = reference(inv_s, ca), evaluate(inv_s, ca, torch.float32)
        err = max(err, float(np.abs(f32[key] - ref[key]).max()))
        ref_max = max(ref_max, float(np.abs(ref[key]).max()))
    return 4.0 * err + 1e-7 * ref_max, err


# ---- the op composed with the compositors: rays whose SDF is a line through zero, on the ray layout of tests/composite_geo_cases.py ----
RAY_INV_S, RAY_COS_ANNEAL = 20.0, 1.0


@functools.lru_cache(maxsize=None)
def ray_case():
    """composite_geo_cases.ray_table(False)'s rays, deltas and colours with, per ray, sdf = 0.1 - k t (t = the compositor's sample
    distance, k = 0.2 / t_end: the ray enters at +0.1, crosses the surface half way and leaves at -0.1), normals = -k dirs (the gradient of that
    SDF along the ray) and one unit direction per ray.  At inv_s = 20 the opacity of a whole crossing is ~0.86: no ray reaches T_thresh
    (asserted by the CPU test).  Rows no ray owns are padding.  -> dict of float64 / int32 numpy arrays"""
    import composite_geo_cases as geo
    t = geo.ray_table(False)
    rng = np.random.default_rng(5)
    n_rows = len(t['sigmas'])
    sdf, normals, dirs = np.zeros(n_rows), np.zeros((n_rows, 3)), np.zeros((n_rows, 3))
    dirs[:, 2] = 1.0
    for _, off, num in t['rays']:
        if num == 0 or off + num > n_rows:
            continue
        sl = slice(int(off), int(off) + int(num))
        ts = np.cumsum(t['deltas'][sl, 1])
        k = 0.2 / ts[-1]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        sdf[sl], dirs[sl], normals[sl] = 0.1 - k * ts, d, -k * d
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return dict(sdf=f32(sdf), normals=f32(normals), dirs=f32(dirs), deltas=t['deltas'], rgbs=t['rgbs'], rays=t['rays'])


def ray_sigmas(dtype):
    """`definition` on ray_case() at `dtype` on the CPU -> float64 numpy [M]"""
    r = ray_case()
    a = lambda k: torch.tensor(r[k]).to(dtype)
    return definition(a('sdf'), a('normals'), a('dirs'), a('deltas'), torch.tensor([RAY_INV_S], dtype=dtype), RAY_COS_ANNEAL).double().numpy()


@functools.lru_cache(maxsize=None)
def ray_literal():
    """the float64 NeuS rendering of ray_case() with literal alphas, w_i = alpha_i prod_{j<i} (1 - alpha_j) over every sample of a fitting ray
    -> dict weights_sum [N], depth [N], image [N,3], min_T (the smallest transmittance behind any ray)"""
    r = ray_case()
    a = lambda k: torch.from_numpy(r[k])
    alpha = literal_alpha(a('sdf'), a('normals'), a('dirs'), a('deltas')[:, 0], torch.tensor(RAY_INV_S, dtype=torch.float64), RAY_COS_ANNEAL).numpy()
    N = len(r['rays'])
    out = dict(weights_sum=np.zeros(N), depth=np.zeros(N), image=np.zeros((N, 3)), min_T=1.0)
    for index, off, num in r['rays']:
        if num == 0 or off + num > len(alpha):
            continue
        sl = slice(int(off), int(off) + int(num))
        T = np.concatenate([[1.0], np.cumprod(1.0 - alpha[sl])])
        w = alpha[sl] * T[:-1]
        out['weights_sum'][index], out['depth'][index] = w.sum(), (w * np.cumsum(r['deltas'][sl, 1])).sum()
        out['image'][index] = (w[:, None] * r['rgbs'][sl]).sum(0)
        out['min_T'] = min(out['min_T'], float(T[-1]))
    return out


@functools.lru_cache(maxsize=None)
def ray_yardstick(key):
    """bound of `key` (weights_sum, depth, image) for sdf_sigmas -> compositor in fp32: 4 x the float32 CPU error of "definition -> cumprod
    compositing" (composite_geo_cases.prefix_form on the float32 definition's sigmas) against ray_literal() + 1e-7 max|ref|"""
    import composite_geo_cases as geo
    r, ref = ray_case(), ray_literal()
    zero = {k: np.zeros_like(v) for k, v in geo.upstream().items()}
    f32 = geo.prefix_form(ray_sigmas(torch.float32).astype(np.float32), r['rgbs'].astype(np.float32), r['deltas'].astype(np.float32), r['rays'], zero,
                          torch.float32)
    err = float(np.abs(f32[key] - ref[key]).max())
    return 4.0 * err + 1e-7 * float(np.abs(ref[key]).max()), err
