"""Cost of the geometry compositor (csrc/raymarching.hip: k_composite_train_geo_fwd / _bwd) at the headline step's shape,
4096 rays and about 2.6e5 samples in fp32: the median time of one call of
  ngp_composite_rays_train_forward / _backward            (k_composite_train_fwd / _bwd, the plain compositor),
  ngp_composite_rays_train_geo_forward / _backward        (+ differentiable depth and the distortion, all four upstream gradients),
and of the PyTorch formulation of what the geo op adds -- the per-sample weights recomputed with torch ops from a segmented cumsum, depth
and the EffDistLoss prefix sums on them, forward and autograd backward of sum(g_depth * depth + g_dist * distortion) (no T_thresh stop: it
composites every sample).  The candidates are timed alternately inside every repetition, HIP events around `batch` back-to-back calls, after warm-up (kernel-only
times: run it under `rocprofv3 --kernel-trace --stats`).  One JSON line.

    python tools/bench_composite_geo.py [--rays 4096] [--mean-samples 64] [--iters 200] [--warmup 20] [--batch 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

import torch  # noqa: E402


def _time_us(fn, batch):
    """device time of `batch` back-to-back calls / batch (a single call of these kernels is shorter than its own launch path)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--mean-samples', type=int, default=64)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=10)
    args = ap.parse_args()

    from raymarching import backend as be
    dev = torch.device('cuda')
    gen = torch.Generator(device='cpu').manual_seed(0)
    N = args.rays
    counts = torch.randint(args.mean_samples // 4, args.mean_samples * 7 // 4 + 1, (N,), generator=gen)
    offsets = torch.cumsum(counts, 0) - counts
    M = int(counts.sum())
    rays = torch.stack([torch.randperm(N, generator=gen), offsets, counts], 1).int().to(dev)
    rand = lambda *shape: torch.rand(*shape, generator=gen).to(dev)
    sigmas = rand(M) * 8.0          # optical depth ~ 4 per 64 samples: most rays end near weights_sum = 1 without the early stop
    rgbs = rand(M, 3)
    deltas = (rand(M, 2) * 0.015 + 0.001).contiguous()
    T_thresh = 1e-4
    g_ws, g_depth, g_img, g_dist = rand(N), rand(N), rand(N, 3), rand(N)
    ws, depth, dist, img = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, 3, device=dev)
    gs, gc = torch.zeros(M, device=dev), torch.zeros(M, 3, device=dev)

    ray_id = torch.repeat_interleave(torch.arange(N, device=dev), counts.to(dev))
    first = offsets.to(dev)[ray_id]

    def seg_cumsum(v):  # inclusive prefix sum inside each ray
        c = torch.cumsum(v, 0)
        return c - (c - v)[first]

    def torch_formulation():
        s = sigmas.detach().requires_grad_()
        od = s * deltas[:, 0]
        od_incl = seg_cumsum(od)
        w = (1.0 - torch.exp(-od)) * torch.exp(-(od_incl - od))
        t = seg_cumsum(deltas[:, 1])
        wt = w * t
        W_lt, D_lt = seg_cumsum(w) - w, seg_cumsum(wt) - wt
        per = 2.0 * w * (t * W_lt - D_lt) + (1.0 / 3.0) * w * w * deltas[:, 0]
        d = torch.zeros(N, device=dev).index_add_(0, ray_id, wt)
        L = torch.zeros(N, device=dev).index_add_(0, ray_id, per)
        (g_depth * d + g_dist * L).sum().backward()

    calls = {
        'k_composite_train_fwd_us': lambda: be.composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, ws, depth, img),
        'k_composite_train_geo_fwd_us': lambda: be.composite_rays_train_geo_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, ws, depth, img, dist),
        'k_composite_train_bwd_us': lambda: be.composite_rays_train_backward(g_ws, g_img, sigmas, rgbs, deltas, rays, ws, img, M, N, T_thresh, gs, gc),
        'k_composite_train_geo_bwd_us': lambda: be.composite_rays_train_geo_backward(g_ws, g_depth, g_img, g_dist, sigmas, rgbs, deltas, rays, ws,
                                                                                    depth, img, dist, M, N, T_thresh, gs, gc),
        'torch_depth_and_distortion_fwd_bwd_us': torch_formulation,
    }
    calls['k_composite_train_geo_fwd_us']()   # the saved outputs the backward calls read
    times = {k: [] for k in calls}
    for it in range(args.warmup + args.iters):
        for name, fn in calls.items():       # alternate the candidates inside every repetition
            us = _time_us(fn, args.batch)
            if it >= args.warmup:
                times[name].append(us)
    result = {'rays': N, 'samples': M, 'iters': args.iters}
    result.update({k: round(statistics.median(v), 1) for k, v in times.items()})
    result['geo_fwd_over_plain'] = round(result['k_composite_train_geo_fwd_us'] / result['k_composite_train_fwd_us'], 2)
    result['geo_bwd_over_plain'] = round(result['k_composite_train_geo_bwd_us'] / result['k_composite_train_bwd_us'], 2)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
