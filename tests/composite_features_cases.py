"""Cases and references shared by tests/test_composite_features_abi.py (CPU) and tests/test_gpu_composite_features.py (GPU): the feature
compositor raymarching.composite_rays_train_features.

The ray table, its two variants and `live_counts` are those of tests/composite_geo_cases.py, unchanged.  On top of them, per channel count C:
  feats(C)        [M,C] uniform(-1, 1) rounded through float16, so the fp16, fp32 and fp64 paths see the same numbers
  upstream(C)     [N,C] uniform(-1, 1), the gradient of the output
  definition      out[index, c] = sum_i w_i feats[offset + i, c] over the live samples in a float64 per-ray loop, gradients by autograd
  closed_form     the formulas the kernels evaluate (forward and single-sweep backward, the ray total Q from the saved output) in plain torch
                  at a chosen dtype: in float32 the yardstick of the fp32 kernels' rounding error, in float64 a check of the formulas
CHANNELS are the counts where a samples-per-pass or channel-block lane layout changes shape: 64 // C = 64, 21, 12, 3, 2, 1; exactly one
full block of 64; a block of one (65); three blocks (130)."""
import functools

import numpy as np
import torch

from composite_geo_cases import M, PERM, RAYS, T_THRESH, live_counts, ray_table  # noqa: F401  (re-exported for the two test files)

N = len(RAYS)
CHANNELS = (1, 3, 5, 21, 22, 33, 64, 65, 130)
KEYS = ('out', 'grad_sigmas', 'grad_feats')


@functools.lru_cache(maxsize=None)
def feats(C):
    """[M,C] float64 holding float16-representable values"""
    return np.random.default_rng(4100 + C).uniform(-1, 1, (M, C)).astype(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def upstream(C):
    return np.random.default_rng(9 + C).uniform(-1, 1, (N, C))


@functools.lru_cache(maxsize=None)
def table_live(early):
    t = ray_table(early)
    return live_counts(t['sigmas'], t['deltas'], t['rays'])


def dead_rows(early):
    """rows no ray composites: behind an early stop, the overflowing ray's rows, the padding"""
    dead = np.ones(M, bool)
    for (_, off, _), k in zip(ray_table(early)['rays'], table_live(early)):
        dead[off:off + k] = False
    return dead


@functools.lru_cache(maxsize=None)
def definition(early, C):
    """float64 definition, ray by ray, with the gradients of sum(upstream(C) * out) by autograd -> dict of numpy arrays (KEYS)"""
    t = ray_table(early)
    s = torch.tensor(t['sigmas'], requires_grad=True)
    f = torch.tensor(feats(C), requires_grad=True)
    dl = torch.tensor(t['deltas'])
    rows = [torch.zeros(C, dtype=torch.float64)] * N
    for (index, off, _), k in zip(t['rays'], table_live(early)):
        if k == 0:
            continue
        sl = slice(int(off), int(off) + k)
        alpha = 1.0 - torch.exp(-s[sl] * dl[sl, 0])
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha[:-1]]), 0)
        rows[index] = ((alpha * T)[:, None] * f[sl]).sum(0)
    out = torch.stack(rows)
    gs, gf = torch.autograd.grad((torch.tensor(upstream(C)) * out).sum(), (s, f))
    return dict(out=out.detach().numpy(), grad_sigmas=gs.numpy(), grad_feats=gf.numpy())


@functools.lru_cache(maxsize=None)
def closed_form(early, C, dtype):
    """The kernels' formulas in plain torch ops at `dtype` on the CPU:
         grad_feats[i, c] = w_i g[c],   q_i = sum_c g[c] feats[i, c],   Q = sum_c g[c] out[c]
         grad_sigmas[i]   = d0_i (T_{i+1} q_i - (Q - sum_{j<=i} w_j q_j))
    -> dict of float64 numpy arrays (KEYS)"""
    t = ray_table(early)
    s, dl, f, up = (torch.tensor(np.asarray(a)).to(dtype) for a in (t['sigmas'], t['deltas'], feats(C), upstream(C)))
    res = dict(out=torch.zeros(N, C, dtype=dtype), grad_sigmas=torch.zeros_like(s), grad_feats=torch.zeros_like(f))
    for (index, off, _), k in zip(t['rays'], table_live(early)):
        if k == 0:
            continue
        sl = slice(int(off), int(off) + k)
        d0 = dl[sl, 0]
        alpha = 1.0 - torch.exp(-s[sl] * d0)
        T_after = torch.cumprod(1.0 - alpha, 0)
        w = alpha * torch.cat([torch.ones(1, dtype=dtype), T_after[:-1]])
        out = (w[:, None] * f[sl]).sum(0)
        g = up[index]
        q = (f[sl] * g[None, :]).sum(1)
        res['out'][index] = out
        res['grad_feats'][sl] = w[:, None] * g[None, :]
        res['grad_sigmas'][sl] = d0 * (T_after * q - ((g * out).sum() - torch.cumsum(w * q, 0)))
    return {k: v.to(torch.float64).numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def yardstick(early, C, key):
    """bound of the fp32 kernels' error in `key`: 4 x the max error of closed_form in float32 against the float64 definition on the same inputs
    + 1e-7 of the largest reference value -- the rule of composite_geo_cases.yardstick.  -> (bound, measured float32 error)"""
    ref = definition(early, C)[key]
    err = float(np.abs(closed_form(early, C, torch.float32)[key] - ref).max())
    return 4.0 * err + 1e-7 * float(np.abs(ref).max()), err
