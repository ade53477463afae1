"""Cost of the geometry losses in the fused training step (csrc/raymarching.hip: k_composite_train_geo_loss_bwd).

Kernel part, at the headline step's shape (4096 rays, about 2.6e5 samples in fp32; the synthetic ray table of tools/bench_composite_geo.py):
the median time of
  ngp_composite_train_geo_loss_backward                    (the one launch, lambda_distortion and lambda_depth > 0),
  the chain it replaces                                    (geo forward -> finish in torch -> ngp_pipeline_mse_loss -> the per-ray gradients
                                                            in torch -> geo backward into zeroed buffers -> rgb backward),
  ngp_composite_train_loss_backward                        (the MSE-only launch of the headline step),
each with the loss summed in the launch and left to a later one (`_deferred`: what the training step does).  The candidates are timed
alternately inside every repetition, HIP events around `batch` back-to-back calls, after warm-up.

Step part (--steps > 0), bench.py's single-GPU workload (synthetic scene, 4096 rays, perturb, NGPAdam, lookahead, table Adam in the grid
backward): ms per step over `--steps` steps, median of `--repeats` windows, of the graph-replayed step without and with
geo_loss=GeoLoss(lambda_distortion), and of the autograd step it replaces (model.render(geo=True) + lambda * distortion.mean()), eager and
captured.  One JSON line.

    python tools/bench_fused_geo.py [--rays 4096] [--mean-samples 64] [--iters 200] [--warmup 20] [--batch 10] [--steps 256] [--repeats 3]
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
    """device time of `batch` back-to-back calls / batch (a single call of these kernels is shorter than its own launch path)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch


def kernel_part(args):
    import _ngp_capi as capi
    lib, st = capi.lib, capi.stream()
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
    T, bg = 1e-4, 1.0
    nears = rand(N) * 0.4 + 0.1
    fars = nears + 1.0 + rand(N) * 2.0
    target, z, m = rand(N, 3), rand(N) * 2.0, rand(N)
    scale = torch.tensor([1024.0], device=dev)
    lam_dist, lam_depth = 0.01, 0.1
    f = lambda *shape: torch.empty(*shape, device=dev)
    ws, image, depth, draw, dist, iraw = f(N), f(N, 3), f(N), f(N), f(N), f(N, 3)
    loss, err, gimg = f(1), f(N), f(N, 3)
    gs, g16, grgb = f(M), torch.empty(M, 16, device=dev, dtype=torch.half), f(M, 3)
    mws = torch.zeros(lib.ngp_march_rays_train_workspace_bytes(N) // 4, dtype=torch.int32, device=dev)
    mws[0] = M
    mws_bytes = mws.numel() * 4
    P = lambda t: t.data_ptr()

    def fused(loss_ptr):
        capi.check(lib.ngp_composite_train_geo_loss_backward(P(sigmas), P(rgbs), P(deltas), P(rays), M, N, T, 1, bg, None, P(nears), P(fars), P(target),
                                                             lam_dist, lam_depth, P(z), P(m), P(scale), P(ws), P(image), P(depth), P(draw), P(dist),
                                                             loss_ptr, P(err), P(gs), P(g16), P(mws), mws_bytes, st))

    def plain(loss_ptr):
        capi.check(lib.ngp_composite_train_loss_backward(P(sigmas), P(rgbs), P(deltas), P(rays), M, N, T, 1, bg, None, P(nears), P(fars), P(target),
                                                         P(scale), P(ws), P(image), P(depth), loss_ptr, P(err), P(gs), P(g16), P(mws), mws_bytes, st))

    two_ld_over_n = 2.0 * lam_depth / N

    def chain():
        capi.check(lib.ngp_composite_rays_train_geo_forward(P(sigmas), P(rgbs), P(deltas), P(rays), M, N, T, P(ws), P(draw), P(iraw), P(dist), st))
        img = iraw + (1.0 - ws)[:, None] * bg
        capi.check(lib.ngp_pipeline_mse_loss(P(img), P(target), 3 * N, P(scale), P(loss), P(gimg), st))
        span = (fars - nears).clamp_min(1.1754944e-38)
        gw = -(gimg.sum(1) * bg)
        gl = (lam_dist / N / span) * scale
        dz = draw - z
        gd = (two_ld_over_n * m * dz) * scale
        total = loss + (lam_dist * (dist / span) + lam_depth * (m * dz * dz)).mean()   # the loss value
        gs.zero_()
        grgb.zero_()
        capi.check(lib.ngp_composite_rays_train_geo_backward(P(gw), P(gd), P(gimg), P(gl), P(sigmas), P(rgbs), P(deltas), P(rays), P(ws), P(draw), P(iraw),
                                                             P(dist), M, N, T, P(gs), P(grgb), st))
        capi.check(lib.ngp_pipeline_rgb_backward(P(grgb), P(rgbs), P(g16), M, st))
        return total

    calls = {
        'geo_loss_bwd_us': lambda: fused(P(loss)), 'geo_loss_bwd_deferred_us': lambda: fused(None),
        'plain_loss_bwd_us': lambda: plain(P(loss)), 'plain_loss_bwd_deferred_us': lambda: plain(None),
        'chain_us': chain,
    }
    times = {k: [] for k in calls}
    for it in range(args.warmup + args.iters):
        for name, fn in calls.items():       # alternate the candidates inside every repetition
            us = _time_us(fn, args.batch)
            if it >= args.warmup:
                times[name].append(us)
    res = {'rays': N, 'samples': M, 'iters': args.iters}
    res.update({k: round(statistics.median(v), 1) for k, v in times.items()})
    res['geo_over_plain'] = round(res['geo_loss_bwd_us'] / res['plain_loss_bwd_us'], 2)
    res['geo_over_plain_deferred'] = round(res['geo_loss_bwd_deferred_us'] / res['plain_loss_bwd_deferred_us'], 2)
    res['chain_over_geo'] = round(res['chain_us'] / res['geo_loss_bwd_us'], 2)
    return res


def step_part(args):
    import raymarching
    import synthetic_scene as sc
    from fused import GeoLoss
    from graph import GraphedTrainStep, mse_loss
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
    dev = torch.device('cuda')
    lam = 0.01
    kw = dict(staged=False, bg_color=1, perturb=True, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    pool = []
    for k in range(16):
        o, d, gt = sc.training_batch(args.rays, seed=k)
        pool.append((torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)))

    def run(mode):
        torch.manual_seed(0)
        model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).to(dev)
        occ = torch.from_numpy(sc.occupancy_density()).to(dev)
        model.train()
        model.density_grid.copy_(occ)
        model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
        bits = model.density_bitfield.clone()
        model.iter_density = 16
        model.mean_density = float(occ.clamp(min=0).mean())
        opt = NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)

        def keep(m):
            m.density_grid.copy_(occ)
            m.density_bitfield.copy_(bits)

        geo = GeoLoss(lambda_distortion=lam)
        if mode in ('graph_mse', 'graph_geo_loss'):
            st = GraphedTrainStep(model, opt, None, args.rays, kw, after_update=keep, lookahead=True, fused_table_adam=True,
                                  geo_loss=geo if mode == 'graph_geo_loss' else None)
        elif mode == 'autograd_geo_graph':   # the captured module-by-module step with the term in loss_fn
            st = GraphedTrainStep(model, opt, None, args.rays, dict(kw, geo=True), after_update=keep,
                                  loss_fn=lambda out, t: mse_loss(out, t) + lam * out['distortion'].float().mean())
        else:                                # 'autograd_geo_eager': the same, launch by launch
            st = GraphedTrainStep(model, opt, None, args.rays, kw, after_update=keep, geo_loss=geo)
        n = [0]

        def step():
            b, nxt = pool[n[0] % 16], pool[(n[0] + 1) % 16]
            n[0] += 1
            if mode == 'autograd_geo_eager':
                if st.global_step % 16 == 0:
                    st._update_extra_state()
                    keep(model)
                loss = st._eager(*b)
                st.global_step += 1
                return loss
            return st.step(*b, next_rays=nxt) if st.lookahead else st.step(*b)

        for _ in range(17):
            step()
        if mode != 'autograd_geo_eager':
            st.precapture()
        for _ in range(47):
            step()
        windows = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step()
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) * 1e3 / args.steps)
        out = {'ms_per_step': round(statistics.median(windows), 4), 'windows_ms': [round(w, 4) for w in windows], 'final_loss': round(float(loss), 6),
               'used_direct': bool(st.used_direct), 'captures': st.n_captures, 'capture_error': st.capture_error}
        st.close()
        return out

    return {mode: run(mode) for mode in ('graph_mse', 'graph_geo_loss', 'autograd_geo_graph', 'autograd_geo_eager')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--mean-samples', type=int, default=64)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--steps', type=int, default=256, help='steps per timed window of the training-step part (0: kernel part only)')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fused_geo: needs a GPU (a time taken elsewhere says nothing)')
    result = {'device': torch.cuda.get_device_name(0), 'kernels': kernel_part(args)}
    if args.steps > 0:
        result['steps_per_window'] = args.steps
        result['step'] = step_part(args)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
