"""numpy model of the error-map kernels (csrc/error_map.hip, include/ngp_hip.h: ngp_error_map_draw / ngp_error_map_update): the hash
words, the race keys in float64, the selection from given fp32 keys, the fp32 refinement to pixels and the fp32 EMA update -- shared by
tests/test_error_map_cases.py (the model draws the stated distribution; CPU) and tests/test_gpu_error_map.py (the kernels are the model)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
FLT_MAX = float(np.finfo(np.float32).max)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mix(x):
    """the finaliser of seeded_noise (raymarching.hip), mod 2^32, on uint64 carriers"""
    x = _u64(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def word(i, b, k, s):
    """word(i, b, k) under seed s (arrays broadcast) -> uint64 holding 32 bits"""
    i, b, k, s = _u64(i), _u64(b), _u64(k), _u64(s)
    inner = mix(((i * np.uint64(0x9E3779B9)) & M32) ^ ((s * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & M32))
    return mix(inner ^ ((b * np.uint64(0xC2B2AE35) + k * np.uint64(0x165667B1) + np.uint64(0x27D4EB2F)) & M32))


def uniforms(i, b, s):
    """u_i: an odd 24-bit integer / 2^24 -- exact in fp32, strictly inside (0, 1); returned as float64 (same value)"""
    w = word(i, b, 0, s)
    return (((w >> np.uint64(9)) << np.uint64(1)) | np.uint64(1)).astype(np.float64) * 2.0 ** -24


def drawable(weights):
    weights = np.asarray(weights, np.float32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(weights) & (weights > 0)


def keys64(weights, b, s):
    """float64 race keys of one image's fp32 weights: -log(u) / w, +inf for an undrawable cell"""
    weights = np.asarray(weights, np.float32)
    ok = drawable(weights)
    u = uniforms(np.arange(weights.shape[-1]), b, s)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return np.where(ok, -np.log(u) / np.where(ok, weights.astype(np.float64), 1.0), np.inf)


def select(keys32, N):
    """the N cells smallest by (key bits, cell index), ascending cell order"""
    keys32 = np.ascontiguousarray(keys32, dtype=np.float32)
    order = np.lexsort((np.arange(keys32.size), keys32.view(np.uint32)))[:N]
    return np.sort(order).astype(np.int64)


def refine(cells, b, s, res, H, W):
    """fp32 refinement of drawn cells to pixel indices row * W + col (plain fp32 multiplies and adds, no fma)"""
    f = np.float32
    cells = np.asarray(cells, np.int64)
    cell_h, cell_w = f(H) / f(res), f(W) / f(res)
    r = (word(cells, b, 1, s) >> np.uint64(8)).astype(f) * f(2.0 ** -24)
    c = (word(cells, b, 2, s) >> np.uint64(8)).astype(f) * f(2.0 ** -24)
    fr = (cells // res).astype(f) * cell_h + r * cell_h
    fc = (cells % res).astype(f) * cell_w + c * cell_w
    assert fr.dtype == f and fc.dtype == f
    row = np.minimum(fr.astype(np.int64), H - 1)
    col = np.minimum(fc.astype(np.int64), W - 1)
    return row * W + col


def update(row, coarse, image, target, keep=0.1, take=0.9):
    """the fp32 EMA update of one map row at cells `coarse` (no duplicates among the in-range ones); out-of-range cells skip their ray"""
    f = np.float32
    row = np.array(row, f)
    coarse = np.asarray(coarse, np.int64)
    e = np.asarray(image, f) - np.asarray(target, f)
    err = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) / f(3.0)
    ok = (coarse >= 0) & (coarse < row.size)
    c = coarse[ok]
    assert np.unique(c).size == c.size
    row[c] = f(keep) * row[c] + f(take) * err[ok]
    assert row.dtype == f
    return row


# ---- the model's draw and three deliberately wrong variants (test_error_map_cases.py: each fails a distribution check) ----
def draw(weights, N, b, s):
    """the stated draw in float64: the N cells smallest by (key, index)"""
    k = keys64(weights, b, s)
    return np.sort(np.lexsort((np.arange(k.size), k))[:N])


def draw_unweighted(weights, N, b, s):
    return draw(np.ones_like(np.asarray(weights, np.float32)), N, b, s)


def draw_uniform_keys(weights, N, b, s):
    """key = u / w instead of -log(u) / w"""
    weights = np.asarray(weights, np.float32)
    k = uniforms(np.arange(weights.size), b, s) / weights.astype(np.float64)
    return np.sort(np.lexsort((np.arange(k.size), k))[:N])


def draw_with_replacement(weights, N, b, s):
    """N independent draws proportional to the weights (inverse CDF on the same uniforms): the set of cells hit"""
    weights = np.asarray(weights, np.float64)
    cdf = np.cumsum(weights) / weights.sum()
    return np.unique(np.minimum(np.searchsorted(cdf, uniforms(np.arange(N), b, s)), weights.size - 1))


def inclusion_counts(fn, weights, N, b, seeds):
    counts = np.zeros(len(weights), np.int64)
    for s in seeds:
        counts[fn(weights, N, b, s)] += 1
    return counts


def inclusion_probabilities_n2(weights):
    """exact P(cell i is among the first two of successive sampling without replacement proportional to the weights)"""
    w = np.asarray(weights, np.float64)
    p = w / w.sum()
    out = p.copy()
    for i in range(w.size):
        for j in range(w.size):
            if j != i:
                out[i] += p[j] * w[i] / (w.sum() - w[j])
    return out


def binomial_z(counts, n, p):
    p = np.asarray(p, np.float64)
    return (np.asarray(counts, np.float64) - n * p) / np.sqrt(n * p * (1.0 - p))
