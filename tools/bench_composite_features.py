"""Cost of compositing C per-sample feature channels along training rays (csrc/raymarching.hip: k_composite_feat_fwd / _bwd).

At M = 262 144 samples over N = 4096 rays (64 per ray, so every sample row is full), C in {3, 16, 64}, fp32 and fp16 features, forward +
backward through autograd:
  A  raymarching.composite_rays_train_features                               (one launch each way)
  B  what a user had before it: ceil(C / 3) x (feats[:, 3k:3k+3].contiguous() -> composite_rays_train -> backward), the channels padded to
     a multiple of 3; fp16 features are up-cast first (composite_rays_train casts its inputs to fp32).
A and B are timed alternately inside every repetition, HIP events around `batch` back-to-back forward + backward pairs, after warm-up; the
medians over the repetitions are reported.  The whole A/B run is repeated `--runs` times in the process: the spread of the medians across
the runs is what a difference between A and B has to exceed.  For A the forward and the backward are also timed alone and set against the
bytes the algorithm needs (e: the feature element size),
  forward   M (4 + 8) + M C e + N C 4            backward   M (4 + 8) + 2 M C e + N C 8 + M 4,
as achieved bytes/s and as a share of the HBM peak (--peak-tbs, 8 TB/s for MI355X).  One JSON line.

    python tools/bench_composite_features.py [--rays 4096] [--samples 64] [--iters 30] [--warmup 5] [--batch 5] [--runs 3]
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
    """device time of `batch` back-to-back calls / batch"""
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
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    args = ap.parse_args()
    import raymarching
    from raymarching import backend

    dev = torch.device('cuda')
    gen = torch.Generator(device='cpu').manual_seed(0)
    N, K = args.rays, args.samples
    M = N * K
    rays = torch.stack([torch.randperm(N, generator=gen), torch.arange(N) * K, torch.full((N,), K)], 1).int().to(dev)
    rand = lambda *shape: torch.rand(*shape, generator=gen).to(dev)
    sigmas = (rand(M) * 4.0).requires_grad_()     # optical depth ~ 1 per ray: no early stop, every sample is composited
    deltas = (rand(M, 2) * 0.015 + 0.001).contiguous()
    T = 1e-4
    result = dict(rays=N, samples=M, iters=args.iters, batch=args.batch, runs=args.runs, cases=[])
    # bring the clocks and the allocator up before the first case (its first run was up to twice as slow as its third without this)
    busy = rand(M, 64)
    for _ in range(400):
        busy = busy * 1.0001 + 0.5
    torch.cuda.synchronize()

    for C in (3, 16, 64):
        for dtype in (torch.float32, torch.float16):
            e = 2 if dtype == torch.float16 else 4
            feats = (rand(M, C) * 2 - 1).to(dtype).requires_grad_()
            up = rand(N, C) * 2 - 1
            groups = (C + 2) // 3
            up3 = torch.zeros(N, groups * 3, device=dev)
            up3[:, :C] = up
            pad = groups * 3 - C

            def run_a():
                sigmas.grad = feats.grad = None
                out = raymarching.composite_rays_train_features(sigmas, feats, deltas, rays, T)
                out.backward(up)

            def run_b():
                sigmas.grad = feats.grad = None
                f = feats.float()
                if pad:
                    f = torch.nn.functional.pad(f, (0, pad))
                outs = [raymarching.composite_rays_train(sigmas, f[:, 3 * k:3 * k + 3].contiguous(), deltas, rays, T)[2] for k in range(groups)]
                torch.autograd.backward(outs, [up3[:, 3 * k:3 * k + 3] for k in range(groups)])

            # A's two launches alone, on preallocated buffers
            out = torch.empty(N, C, device=dev)
            gs, gf = torch.zeros(M, device=dev), torch.zeros(M, C, device=dev, dtype=dtype)
            s0, f0 = sigmas.detach(), feats.detach()
            fwd = lambda: backend.composite_rays_train_features_forward(s0, f0, deltas, rays, M, N, C, T, out)
            bwd = lambda: backend.composite_rays_train_features_backward(up, s0, f0, deltas, rays, out, M, N, C, T, gs, gf)

            medians = {k: [] for k in ('A', 'B', 'fwd', 'bwd')}
            for _ in range(args.runs):
                for fn in (run_a, run_b, fwd, bwd):
                    for _ in range(args.warmup):
                        fn()
                t = {k: [] for k in medians}
                for _ in range(args.iters):
                    for k, fn in (('A', run_a), ('B', run_b), ('fwd', fwd), ('bwd', bwd)):
                        t[k].append(_time_us(fn, args.batch))
                for k in medians:
                    medians[k].append(statistics.median(t[k]))
            bytes_f = M * 12 + M * C * e + N * C * 4
            bytes_b = M * 12 + 2 * M * C * e + N * C * 8 + M * 4
            med = {k: statistics.median(v) for k, v in medians.items()}
            spread = {k: max(v) - min(v) for k, v in medians.items()}
            result['cases'].append(dict(
                C=C, feats='fp16' if e == 2 else 'fp32', launches_B=2 * groups,
                A_us=round(med['A'], 1), B_us=round(med['B'], 1), A_spread_us=round(spread['A'], 1), B_spread_us=round(spread['B'], 1),
                A_runs_us=[round(v, 1) for v in medians['A']], B_runs_us=[round(v, 1) for v in medians['B']],
                A_below_B_by_more_than_the_spread=bool(max(medians['A']) + max(spread['A'], spread['B']) < min(medians['B'])),
                fwd_us=round(med['fwd'], 1), bwd_us=round(med['bwd'], 1), fwd_bytes=bytes_f, bwd_bytes=bytes_b,
                fwd_tbs=round(bytes_f / med['fwd'] * 1e-6, 3), bwd_tbs=round(bytes_b / med['bwd'] * 1e-6, 3),
                fwd_peak_share=round(bytes_f / med['fwd'] * 1e-6 / args.peak_tbs, 3),
                bwd_peak_share=round(bytes_b / med['bwd'] * 1e-6 / args.peak_tbs, 3)))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
