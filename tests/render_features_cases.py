"""Cases and references shared by tests/test_render_features_cases.py (CPU) and tests/test_gpu_render_features.py (GPU): the feature
compositor of the inference loop, k_composite_rays_feat of csrc/raymarching.hip behind ngp_composite_rays_features / _dev (include/ngp_hip.h,
DESIGN.md 3.12).  Everything about the rays -- the 97-ray tables, the named rays, T_thresh, the margin rule, the three consecutive calls, the
ladder of n_step -- is render_loop_cases'; this module adds the channels.

`features_model`        the definition as a per-ray loop in the statement order of k_composite_rays (render_loop_cases.composite_model with
                        `acc[c] += w * feats[s, c]` in the place of depth / image, nothing written but `out`).  At dtype=np.float64 it is the
                        DEFINITION; at np.float32 every operation is rounded to fp32 (the product and the sum separately: the kernel does
                        not contract them) and exp is evaluated in fp32: the yardstick.  The variants 'le' / 'threshold_first' are
                        composite_model's two deliberately wrong compositors.
`features_table`        composite_table(n_step) + feats [61, n_step, C] uniform in (-1, 1) + a non-zero out0 [97, C]; every feature row at or
                        behind the definition's count[n] is NaN: a kernel that reads behind a ray's break shows it in `out`.
`features_bound`        the rule of render_loop_cases.bound_of: 4 x (float32 model error against the float64 definition) + 1e-7 x max |ref|.
`features_multi_table`  channels for the three calls of multi_call_table(); `run_features_multi` runs them with weights_sum taken from the
                        compositor's state between calls (each feature call BEFORE the compositor's call on the same rows)."""
import functools
import math

import numpy as np

import render_loop_cases as L

CHANNELS_CPU = (1, 3, 33, 256)


def features_model(call, feats, out0, dtype, exp2=False, variant='definition'):
    """-> (out [N,C] at `dtype`: an updated COPY of out0, count [n_alive]: the samples composited per list entry).  `call`: a dict like
    composite_table's (n_alive, n_step, T_thresh, rays_alive, sigmas, deltas, weights_sum); feats [n_alive, n_step, C] or [rows, C]"""
    f = dtype
    n_alive, n_step = call['n_alive'], call['n_step']
    alive = np.asarray(call['rays_alive'], np.int32)
    W = np.array(call['weights_sum'], dtype=f)
    sg, de = np.asarray(call['sigmas'], dtype=f).reshape(-1), np.asarray(call['deltas'], dtype=f).reshape(-1, 2)
    out = np.array(out0, dtype=f).copy()
    ft = np.asarray(feats, dtype=f).reshape(-1, out.shape[1])
    one, thresh = f(1.0), f(call['T_thresh'])
    log2e = f(math.log2(math.e))
    count = np.zeros(n_alive, np.int64)
    for n in range(n_alive):
        index = int(alive[n])
        w_sum, acc = W[index], out[index].copy()
        for step in range(n_step):
            s = n * n_step + step
            d0 = de[s, 0]
            if d0 == 0:
                break
            x = f(-sg[s]) * d0
            alpha = one - (np.exp2(f(x * log2e)) if exp2 else np.exp(x))
            T = one - w_sum
            if variant == 'threshold_first' and T < thresh:
                break
            w = alpha * T
            w_sum = w_sum + w
            acc = acc + w * ft[s]
            count[n] += 1
            if (T <= thresh) if variant == 'le' else (T < thresh):
                break
        out[index] = acc
    assert out.dtype == f
    return out, count


@functools.lru_cache(maxsize=None)
def features_table(n_step, C):
    """-> composite_table(n_step)'s dict (treat as read-only) + C, feats [61, n_step, C] float32 (NaN at and behind each entry's break),
    out0 [97, C] float32 (|out0| in [0.1, 1))"""
    t = L.composite_table(n_step)
    rng = np.random.default_rng(900000 + 1000 * n_step + C)
    feats = L._f32(rng.uniform(-1.0, 1.0, (L.N_ALIVE, n_step, C)))
    out0 = L._f32(rng.uniform(0.1, 1.0, (L.N, C)) * rng.choice([-1.0, 1.0], (L.N, C)))
    count = L.table_reference(n_step)['count']
    for n in range(L.N_ALIVE):
        feats[n, count[n]:] = np.nan
    return dict(t, C=C, feats=feats, out0=out0)


def _bound(ref, f32):
    err = float(np.abs(f32.astype(np.float64) - ref).max())
    return 4.0 * err + 1e-7 * float(np.abs(ref).max()), err


def table_feats(n_step, C, half=False):
    """the table's channels as the kernel sees them: float32, or (half) rounded to float16 -- the fp16 kernel converts at the load, so its
    definition is the definition on the up-cast values"""
    feats = features_table(n_step, C)['feats']
    return feats.astype(np.float16) if half else feats


@functools.lru_cache(maxsize=None)
def features_reference(n_step, C, half=False):
    """the float64 definition on features_table(n_step, C), computed once -> (out, count)"""
    t = features_table(n_step, C)
    return features_model(t, table_feats(n_step, C, half).astype(np.float32), t['out0'], np.float64)


@functools.lru_cache(maxsize=None)
def features_bound(n_step, C, exp2=False, half=False):
    """-> (bound, float32 model error) of features_table(n_step, C)"""
    t = features_table(n_step, C)
    f32, _ = features_model(t, table_feats(n_step, C, half).astype(np.float32), t['out0'], np.float32, exp2=exp2)
    return _bound(features_reference(n_step, C, half)[0], f32)


# ------------------------------------------------------------------------------------------------
# three consecutive calls
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def features_multi_table(C):
    """-> dict: feats (one [n_alive_i, 4, C] float32 array per call of multi_call_table(), NaN at and behind each entry's break in the
    definition), out0 [97, C]"""
    rng = np.random.default_rng(770000 + C)
    out0 = L._f32(rng.uniform(0.1, 1.0, (L.N, C)) * rng.choice([-1.0, 1.0], (L.N, C)))
    feats = []
    for call in L.multi_call_table():
        a = L._f32(rng.uniform(-1.0, 1.0, (call['n_alive'], call['n_step'], C)))
        count = L.run_model(call, np.float64)['count']     # (each call holds the definition's state in front of it)
        for n in range(call['n_alive']):
            a[n, count[n]:] = np.nan
        feats.append(a)
    return dict(feats=feats, out0=out0, C=C)


def run_features_multi(C, dtype, exp2=False):
    """the three calls at `dtype`: per call the feature model on the state in front of the compositor's call, then the compositor's call ->
    (out, [count per call])"""
    calls, tab = L.multi_call_table(), features_multi_table(C)
    state = {k: calls[0][k].astype(dtype) for k in L.KEYS}
    out = tab['out0'].astype(dtype)
    counts = []
    for call, feats in zip(calls, tab['feats']):
        cur = dict(call, **state)
        out, count = features_model(cur, feats, out, dtype, exp2=exp2)
        done = L.run_model(cur, dtype, exp2=exp2)
        state = {k: done[k] for k in L.KEYS}
        counts.append(count)
    return out, counts


@functools.lru_cache(maxsize=None)
def features_multi_bound(C, exp2=False):
    """-> (float64 end `out`, bound, float32 model error)"""
    ref, _ = run_features_multi(C, np.float64)
    f32, _ = run_features_multi(C, np.float32, exp2=exp2)
    return (ref,) + _bound(ref, f32)
