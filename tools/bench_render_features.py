"""Cost of compositing C caller-defined channels in the inference loop (csrc/raymarching.hip: k_composite_rays_feat behind
ngp_composite_rays_features, render(aux_infer=...)).  Two parts, one JSON line each.

--kernel   one loop iteration's compositing at n_alive = 262 144 list entries, n_step in {2, 8}, C in {3, 16, 64}, fp32 and fp16 features:
  A  ngp_composite_rays_features                                              (one launch)
  B  what a user had before it: ceil(C / 3) x (clones of rays_alive, rays_t, weights_sum and a scratch depth, a contiguous slice
     feats[:, 3k:3k+3] (the last one padded to 3, fp16 up-cast), ngp_composite_rays into a per-group [N,3] image) -- the compositor advances
     rays_t and weights_sum and kills rays, so every group needs its own copy of the loop state.
  A and B are timed alternately inside every repetition, HIP events around `batch` back-to-back calls, after warm-up; the medians over the
  repetitions are reported, and the whole A/B run is repeated `--runs` times in the process: the spread of the medians across the runs is
  what a difference has to exceed.  A is also set against the bytes it has to move (e: the feature element size),
      rows (4 + 8) + rows C e + n_alive (8 + 2 C 4),      rows = n_alive n_step,
  as achieved bytes/s and as a share of the HBM peak (--peak-tbs, 8 TB/s for MI355X).
--frame    model.render at 800x800 on the transparent (density_scale 1) and opaque (300) brackets of tools/bench_render.py: without
  aux_infer on the native pair call, without it on the per-stage path (native_loop = False), and with aux_infer at C in {3, 16, 64} (a fixed
  [3,C] linear map of rgbs).  native -> per-stage is the price of leaving the native pair call, which an aux_infer frame pays; per-stage ->
  aux_infer is the callable plus the feature launch, which one probed frame per C splits by stage (HIP events, `_loop_probe`).

    python tools/bench_render_features.py [--kernel] [--frame] [--iters 10] [--warmup 3] [--batch 3] [--runs 3] [--frames 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def kernel_part(args):
    from raymarching import backend
    dev = torch.device('cuda')
    gen = torch.Generator(device='cpu').manual_seed(0)
    rand = lambda *shape: torch.rand(*shape, generator=gen).to(dev)
    n_alive, T = args.alive, 1e-4
    N = n_alive + n_alive // 2                       # the list is a scattered subset of the frame's rays
    alive = torch.randperm(N, generator=gen)[:n_alive].int().to(dev)
    result = dict(part='kernel', n_alive=n_alive, rays=N, iters=args.iters, batch=args.batch, runs=args.runs, cases=[])
    busy = rand(1 << 22)                             # bring the clocks and the allocator up before the first case
    for _ in range(400):
        busy = busy * 1.0001 + 0.5
    torch.cuda.synchronize()
    for n_step in (2, 8):
        rows = n_alive * n_step
        deltas = (rand(rows, 2) * 0.015 + 0.001).contiguous()
        sigmas = rand(rows) * (1.0 / n_step) / deltas[:, 0]     # optical depth ~ 0.5 per call: no ray stops, every row is composited
        rays_t, ws0, depth0 = rand(N), rand(N) * 0.5, rand(N)
        for C in (3, 16, 64):
            groups = (C + 2) // 3
            for dtype in (torch.float32, torch.float16):
                e = 2 if dtype == torch.float16 else 4
                feats = (rand(rows, C) * 2 - 1).to(dtype)
                out = torch.zeros(N, C, device=dev)
                images = [torch.zeros(N, 3, device=dev) for _ in range(groups)]

                def run_a():
                    backend.composite_rays_features(n_alive, n_step, T, alive, sigmas, feats, deltas, ws0, out)

                def run_b():
                    for k in range(groups):
                        a, t, w, d = alive.clone(), rays_t.clone(), ws0.clone(), depth0.clone()
                        f = feats[:, 3 * k:3 * k + 3].float()
                        if f.shape[1] < 3:
                            f = torch.nn.functional.pad(f, (0, 3 - f.shape[1]))
                        backend.composite_rays(n_alive, n_step, T, a, t, sigmas, f.contiguous(), deltas, w, d, images[k])

                medians = {'A': [], 'B': []}
                for _ in range(args.runs):
                    for fn in (run_a, run_b):
                        for _ in range(args.warmup):
                            fn()
                    t = {'A': [], 'B': []}
                    for _ in range(args.iters):
                        t['A'].append(_time_us(run_a, args.batch))
                        t['B'].append(_time_us(run_b, args.batch))
                    for k in medians:
                        medians[k].append(statistics.median(t[k]))
                med = {k: statistics.median(v) for k, v in medians.items()}
                spread = {k: max(v) - min(v) for k, v in medians.items()}
                nbytes = rows * 12 + rows * C * e + n_alive * (8 + 2 * C * 4)
                result['cases'].append(dict(
                    n_step=n_step, C=C, feats='fp16' if e == 2 else 'fp32', launches_B=groups,
                    A_us=round(med['A'], 1), B_us=round(med['B'], 1), A_spread_us=round(spread['A'], 1), B_spread_us=round(spread['B'], 1),
                    A_runs_us=[round(v, 1) for v in medians['A']], B_runs_us=[round(v, 1) for v in medians['B']],
                    A_below_B_by_more_than_the_spread=bool(max(medians['A']) + max(spread['A'], spread['B']) < min(medians['B'])),
                    A_bytes=nbytes, A_tbs=round(nbytes / med['A'] * 1e-6, 3), A_peak_share=round(nbytes / med['A'] * 1e-6 / args.peak_tbs, 3)))
                del feats, out, images
    print(json.dumps(result), flush=True)


def frame_part(args):
    import numpy as np
    import raymarching
    import synthetic_scene as sc
    from nerf.network_ff import NeRFNetwork
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1.0, min_near=0.2, density_thresh=10).to(dev).eval()
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()).to(dev))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    o, d = sc.full_image_rays(seed=0)
    ro, rd = torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev)
    kw = dict(staged=True, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    maps = {C: torch.randn(3, C, device=dev) for C in (3, 16, 64)}
    variants = [('native pair call', True, None), ('per-stage path', False, None)] + [(f'aux_infer C={C}', True, C) for C in maps]
    result = dict(part='frame', rays=int(ro.shape[1]), frames=args.frames, cases=[])
    for scale in (1.0, 300.0):
        model.density_scale = scale
        ref = None
        for name, native, C in variants:
            model.native_loop, model._loop_cache, model._loop_probe = native, None, None
            fn = None if C is None else (lambda x, dd, s, c, W=maps[C]: c @ W)
            times = []
            for _ in range(args.frames + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
                    out = model.render(ro, rd, aux_infer=fn, **kw)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            ref = out['image'] if ref is None else ref
            case = dict(density_scale=scale, variant=name, min_ms=round(min(times[1:]), 3), mean_ms=round(float(np.mean(times[1:])), 3),
                        first_frame_ms=round(times[0], 1), image_identical_to_native=bool(torch.equal(out['image'], ref)))
            if C is not None:   # one probed frame: device time per stage (the events serialise the stages a little: shares, not the frame time)
                model._loop_probe = probe = []
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
                    model.render(ro, rd, aux_infer=fn, **kw)
                torch.cuda.synchronize()
                model._loop_probe = None
                by_stage = {}
                for rec in probe:
                    by_stage[rec[0]] = by_stage.get(rec[0], 0.0) + rec[1].elapsed_time(rec[2])
                case.update(iterations=sum(1 for rec in probe if rec[0] == 'composite_rays'),
                            stage_ms={k: round(v, 3) for k, v in by_stage.items()},
                            aux_finite=bool(torch.isfinite(out['aux']).all()))
            result['cases'].append(case)
    model.native_loop = True
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--frame', action='store_true')
    ap.add_argument('--alive', type=int, default=262144)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=3)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    args = ap.parse_args()
    both = not (args.kernel or args.frame)
    if args.kernel or both:
        kernel_part(args)
    if args.frame or both:
        frame_part(args)


if __name__ == '__main__':
    main()
