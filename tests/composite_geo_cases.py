"""Cases and references shared by tests/test_composite_geo_abi.py (CPU) and tests/test_gpu_composite_geo.py (GPU): the geometry
compositor raymarching.composite_rays_train_geo.

ONE ray table (`ray_table`), in two variants that differ only in the sigmas of two rays:
  early=True   every branch of the kernels: the rays below, one of them saturating inside its first 64-sample row, one whose
               transmittance crosses T_thresh exactly at the row boundary;
  early=False  the same layout with mild sigmas everywhere (all weights_sum < 0.9, asserted on the reference): no sample sits on the
               T_thresh discontinuity, for the gradient tests.
`reference` is the O(K^2) DEFINITION of the distortion in float64 torch on the CPU, per ray in a loop, with gradients by autograd -- independent
of the O(K) prefix form the kernels use.  `prefix_form` is that O(K) form and its closed-form backward in plain torch at a chosen dtype: in
float32 it is the yardstick of the fp32 kernels' rounding error, in float64 a check of the formulas themselves."""
import functools
import math

import numpy as np
import torch

T_THRESH = 1e-4
M = 1600
# (name, sample count); offsets are consecutive in this order, the overflowing ray starts inside the padding
RAYS = [('empty', 0), ('single', 1), ('row-1', 63), ('row', 64), ('row+1', 65), ('three rows', 130), ('long', 300), ('saturating', 300),
        ('boundary', 200), ('overflow', 300)]
NAMES = [n for n, _ in RAYS]
OVERFLOW_OFFSET = 1400               # + 300 > M
BOUNDARY_SIGMA, BOUNDARY_D0 = 7.25, 0.02   # exp(-0.145 * 63) = 1.08e-4 >= T_thresh > exp(-0.145 * 64) = 9.3e-5: the break is after sample 63
PERM = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]  # rays[:, 0]: the output row of each ray


@functools.lru_cache(maxsize=None)
def ray_table(early):
    """-> dict of float64 / int32 numpy arrays: sigmas [M], rgbs [M,3], deltas [M,2], rays [N,3], and `used` (rows owned by a fitting ray)"""
    rng = np.random.default_rng(20240)
    counts = np.array([c for _, c in RAYS])
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
    offsets[NAMES.index('overflow')] = OVERFLOW_OFFSET
    used = int(counts[:-1].sum())
    assert used < OVERFLOW_OFFSET < M < OVERFLOW_OFFSET + counts[-1]
    rays = np.stack([np.array(PERM), offsets, counts], 1).astype(np.int32)
    deltas = np.stack([rng.uniform(0.005, 0.05, M), rng.uniform(0.005, 0.05, M)], 1)
    deltas[used:] = 0.0                                   # trailing padding rows
    sigmas = rng.uniform(0.1, 2.0, M)
    rgbs = rng.uniform(0.0, 1.0, (M, 3))
    for n, (name, num) in enumerate(RAYS[:-1]):
        sl = slice(offsets[n], offsets[n] + num)
        if num:  # optical depth 1.6 over the whole ray: weights_sum = 1 - exp(-1.6) = 0.80, T stays far above T_thresh
            sigmas[sl] *= 1.6 / float((sigmas[sl] * deltas[sl, 0]).sum())
        if early and name == 'saturating':
            sigmas[sl] = 400.0
        if early and name == 'boundary':
            sigmas[sl] = BOUNDARY_SIGMA
            deltas[sl, 0] = BOUNDARY_D0
    # float32-representable values: the fp32 kernels and the float64 reference see the same numbers
    sigmas, rgbs, deltas = (a.astype(np.float32).astype(np.float64) for a in (sigmas, rgbs, deltas))
    return dict(sigmas=sigmas, rgbs=rgbs, deltas=deltas, rays=rays, used=used)


@functools.lru_cache(maxsize=None)
def upstream():
    """random upstream gradients of the four outputs: weights_sum [N], depth [N], image [N,3], distortion [N]"""
    rng = np.random.default_rng(7)
    N = len(RAYS)
    return dict(weights_sum=rng.uniform(-1, 1, N), depth=rng.uniform(-1, 1, N), image=rng.uniform(-1, 1, (N, 3)), distortion=rng.uniform(-1, 1, N))


def live_counts(sigmas, deltas, rays, n_samples=None, T_thresh=T_THRESH):
    """samples each ray composites (plain float64 loop): 0 for an empty or overflowing ray; the sample that drives T below T_thresh is in"""
    n_samples = len(sigmas) if n_samples is None else n_samples
    out = []
    for _, off, num in rays:
        k = 0
        if num and off + num <= n_samples:
            T = 1.0
            for s in range(off, off + num):
                T *= math.exp(-float(sigmas[s]) * float(deltas[s, 0]))
                k += 1
                if T < T_thresh:
                    break
        out.append(k)
    return out


def reference(sigmas, rgbs, deltas, rays, grads=None, T_thresh=T_THRESH):
    """float64 definition, ray by ray: weights_sum, depth, image, distortion = sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 d0_i over the live
    samples; with `grads` (dict like upstream()) also grad_sigmas / grad_rgbs of sum(grads * outputs) by autograd.  -> dict of numpy arrays"""
    s = torch.tensor(np.asarray(sigmas, np.float64), requires_grad=True)
    c = torch.tensor(np.asarray(rgbs, np.float64), requires_grad=True)
    dl = torch.tensor(np.asarray(deltas, np.float64))
    N = len(rays)
    live = live_counts(s.detach().numpy(), dl.numpy(), rays, T_thresh=T_thresh)
    zero = torch.zeros((), dtype=torch.float64)
    W, D, L, I = [zero] * N, [zero] * N, [zero] * N, [torch.zeros(3, dtype=torch.float64)] * N
    for (index, off, _), k in zip(rays, live):
        if k == 0:
            continue
        sl = slice(int(off), int(off) + k)
        d0, t = dl[sl, 0], torch.cumsum(dl[sl, 1], 0)
        alpha = 1.0 - torch.exp(-s[sl] * d0)
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha[:-1]]), 0)
        w = alpha * T
        W[index], D[index], I[index] = w.sum(), (w * t).sum(), (w[:, None] * c[sl]).sum(0)
        L[index] = (w[:, None] * w[None, :] * (t[:, None] - t[None, :]).abs()).sum() + (w * w * d0).sum() / 3.0
    out = dict(weights_sum=torch.stack(W), depth=torch.stack(D), image=torch.stack(I), distortion=torch.stack(L))
    res = {k: v.detach().numpy() for k, v in out.items()}
    res['live'] = live
    if grads is not None:
        loss = sum((torch.tensor(np.asarray(grads[k], np.float64)) * out[k]).sum() for k in out)
        gs, gc = torch.autograd.grad(loss, (s, c), allow_unused=True)
        res['grad_sigmas'] = (torch.zeros_like(s) if gs is None else gs).numpy()
        res['grad_rgbs'] = (torch.zeros_like(c) if gc is None else gc).numpy()
    return res


@functools.lru_cache(maxsize=None)
def table_reference(early):
    """reference(...) of ray_table(early) with the upstream() gradients, computed once"""
    t = ray_table(early)
    return reference(t['sigmas'], t['rgbs'], t['deltas'], t['rays'], upstream())


def prefix_form(sigmas, rgbs, deltas, rays, grads, dtype, T_thresh=T_THRESH):
    """The O(K) form the kernels evaluate, in plain torch ops at `dtype` on the CPU (exp, cumprod, cumsum):
         L = sum_i 2 w_i (t_i W_<i - D_<i) + 1/3 sum_i w_i^2 d0_i
         g_i = 2 (t_i W_<i - D_<i) + 2 ((D - D_<=i) - t_i (W - W_<=i)) + 2/3 w_i d0_i
         d depth / d sigma_i = d0_i (T_{i+1} t_i - (D - D_<=i)),  d L / d sigma_i = d0_i (g_i T_{i+1} - (G - G_<=i)),  G = 2 L
    -> dict of numpy arrays (the keys of `reference`)"""
    s, c, dl = (torch.tensor(np.asarray(a)).to(dtype) for a in (sigmas, rgbs, deltas))
    up = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in grads.items()}
    N = len(rays)
    out = dict(weights_sum=torch.zeros(N, dtype=dtype), depth=torch.zeros(N, dtype=dtype), image=torch.zeros(N, 3, dtype=dtype),
               distortion=torch.zeros(N, dtype=dtype), grad_sigmas=torch.zeros_like(s), grad_rgbs=torch.zeros_like(c))
    live = live_counts(np.asarray(sigmas, np.float64), np.asarray(deltas, np.float64), rays, T_thresh=T_thresh)
    for (index, off, _), k in zip(rays, live):
        if k == 0:
            continue
        sl = slice(int(off), int(off) + k)
        d0, t, col = dl[sl, 0], torch.cumsum(dl[sl, 1], 0), c[sl]
        alpha = 1.0 - torch.exp(-s[sl] * d0)
        T_after = torch.cumprod(1.0 - alpha, 0)
        T_before = torch.cat([torch.ones(1, dtype=dtype), T_after[:-1]])
        w = alpha * T_before
        W_le, D_le = torch.cumsum(w, 0), torch.cumsum(w * t, 0)
        W_lt, D_lt = W_le - w, D_le - w * t
        W, D, img = w.sum(), (w * t).sum(), (w[:, None] * col).sum(0)
        L = (2.0 * w * (t * W_lt - D_lt)).sum() + (w * w * d0).sum() / 3.0
        out['weights_sum'][index], out['depth'][index], out['image'][index], out['distortion'][index] = W, D, img, L
        g = 2.0 * (t * W_lt - D_lt) + 2.0 * ((D - D_le) - t * (W - W_le)) + (2.0 / 3.0) * w * d0
        G_le = torch.cumsum(g * w, 0)
        C_le = torch.cumsum(w[:, None] * col, 0)
        gi, gw, gd, gl = up['image'][index], up['weights_sum'][index], up['depth'][index], up['distortion'][index]
        out['grad_rgbs'][sl] = gi[None, :] * w[:, None]
        out['grad_sigmas'][sl] = d0 * (((T_after[:, None] * col - (img[None, :] - C_le)) * gi[None, :]).sum(1) + gw * (1.0 - W) +
                                       gd * (T_after * t - (D - D_le)) + gl * (g * T_after - (2.0 * L - G_le)))
    return {k: v.to(torch.float64).numpy() for k, v in out.items()}


def yardstick(early, key):
    """bound of the fp32 kernels' error in output `key` on ray_table(early): 4 x the max error of prefix_form in float32 against the float64
    reference on the same inputs (the rounding of the same formulas in the same format; the factor covers __expf against exp and the
    scan order) + 1e-7 of the largest reference value.  -> (bound, measured float32 error)"""
    t = ray_table(early)
    ref = table_reference(early)
    f32 = prefix_form(t['sigmas'].astype(np.float32), t['rgbs'].astype(np.float32), t['deltas'].astype(np.float32), t['rays'], upstream(),
                      torch.float32)
    err = float(np.abs(f32[key] - ref[key]).max())
    return 4.0 * err + 1e-7 * float(np.abs(ref[key]).max()), err
