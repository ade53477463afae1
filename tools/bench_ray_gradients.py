"""Cost of the camera-pose gradients through the training rays (csrc/ray_gradient.hip) at the benchmark step's shape:
4096 rays of the synthetic scene, ~2.6e5 samples.

  (a) the fused training render, forward + backward through autograd, WITHOUT and WITH rays that require grad (the second also runs the
      generic branch of the network backward, ngp_grid_input_gradient, ngp_ray_sample_ts and ngp_ray_points_backward);
  (b) ngp_grid_input_gradient against what the existing route costs EXTRA on the same points and the same fp16 table: the encoder forward
      with dy_dx minus without it, plus the first backward with (dy_dx, grad_inputs) minus without them (k_grid_input_backward rides in that
      call); the plain encoder forward is reported beside them as the yardstick (the kernel is bound by gather issue like the forward).
The variants are timed alternately inside every repetition of one process, HIP events around `batch` back-to-back calls, after a warm-up;
medians over the repetitions and their spread (min .. max) are reported.  One JSON line.

    python tools/bench_ray_gradients.py [--rays 4096] [--iters 60] [--warmup 10] [--batch 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

import numpy as np  # noqa: E402
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


def _alternate(fns, iters, warmup, batch):
    """{name: (median us, min us, max us)} of callables timed alternately"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            t[k].append(_time_us(fn, batch))
    return {k: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=3)
    args = ap.parse_args()
    assert args.iters >= 50, 'at least 50 repetitions'
    import _ngp_capi as capi
    import raymarching
    import synthetic_scene as sc
    from gridencoder.backend import _backend as gb
    from nerf.network_ff import NeRFNetwork

    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1).to(dev)
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-0.5, 0.5)
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.train()
    o, d, gt = sc.training_batch(args.rays, seed=1)
    ro, rd, gtt = torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)
    kw = dict(staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):   # the sample count of this batch (the drop-in branch reads it back)
        model.render(ro, rd, force_all_rays=True, **kw)
    model.mean_count = int(model.step_counter[0, 0].item())
    model.local_step = 0
    result = dict(rays=args.rays, samples=model.mean_count, iters=args.iters, batch=args.batch)

    # bring the clocks and the allocator up before the first case
    busy = torch.rand(1 << 22, device=dev)
    for _ in range(400):
        busy = busy * 1.0001 + 0.5
    torch.cuda.synchronize()

    # ---- (a) the fused training render ----
    def step(ray_grads):
        a, b = ro.clone().requires_grad_(ray_grads), rd.clone().requires_grad_(ray_grads)
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.float16):
            assert model._fused_render_ok(a.view(-1, 3), b.view(-1, 3), 1, False)
            out = model.render(a, b, force_all_rays=False, **kw)
            loss = ((out['image'][0] - gtt) ** 2).mean()
        (loss * 65536.0).backward()

    ta = _alternate({'render_fwd_bwd': lambda: step(False), 'render_fwd_bwd_ray_grads': lambda: step(True)}, args.iters, args.warmup, args.batch)
    result['fused_render'] = {k: dict(median_us=v[0], min_us=v[1], max_us=v[2]) for k, v in ta.items()}
    result['fused_render']['ray_grads_extra_us'] = round(ta['render_fwd_bwd_ray_grads'][0] - ta['render_fwd_bwd'][0], 1)

    # ---- (b) dL/dxyzs: the new kernel against the extra cost of the dy_dx route, same points, same fp16 table ----
    enc = model.encoder
    with torch.no_grad():
        nears, fars = raymarching.near_far_from_aabb(ro[0], rd[0], model.aabb_train, model.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        xyzs, _dirs, _deltas, _rays = raymarching.march_rays_train(ro[0], rd[0], model.bound, model.density_bitfield, model.cascade, model.grid_size,
                                                                   nears, fars, counter, -1, False, 128, True, 0, 1024)
    xyzs = xyzs.contiguous()
    M, L = xyzs.shape[0], int(enc.num_levels)
    S, H = float(np.log2(enc.per_level_scale)), int(enc.base_resolution)
    emb16 = enc.embeddings.detach().half().contiguous()
    offs = enc.offsets
    x01 = ((xyzs + 1.0) / 2.0).contiguous()
    g_enc = (torch.randn(L, M, 2, device=dev) * 0.05).half()
    g_xyzs = torch.empty(M, 3, device=dev)
    out16 = torch.empty(L, M, 2, device=dev, dtype=torch.half)
    dy_dx = torch.empty(M, L * 3 * 2, device=dev, dtype=torch.half)
    g_emb = torch.zeros_like(emb16)
    g_in = torch.zeros(M, 3, device=dev, dtype=torch.half)
    st = capi.stream()

    def new_kernel():
        capi.check(capi.lib.ngp_grid_input_gradient(g_enc.data_ptr(), xyzs.data_ptr(), emb16.data_ptr(), offs.data_ptr(), M, 3, 2, L, S, H, 0, 0, 0,
                                                    capi.NGP_F16, 1.0, g_xyzs.data_ptr(), st))

    fns = {'grid_input_gradient': new_kernel,
           'forward': lambda: gb.grid_encode_forward(x01, emb16, offs, out16, M, 3, 2, L, S, H, None, 0, False, 0),
           'forward_dy_dx': lambda: gb.grid_encode_forward(x01, emb16, offs, out16, M, 3, 2, L, S, H, dy_dx, 0, False, 0),
           'backward': lambda: gb.grid_encode_backward(g_enc, x01, emb16, offs, g_emb, M, 3, 2, L, S, H, None, None, 0, False, 0),
           'backward_dy_dx': lambda: gb.grid_encode_backward(g_enc, x01, emb16, offs, g_emb, M, 3, 2, L, S, H, dy_dx, g_in, 0, False, 0)}
    tb = _alternate(fns, args.iters, args.warmup, args.batch)
    route = (tb['forward_dy_dx'][0] - tb['forward'][0]) + (tb['backward_dy_dx'][0] - tb['backward'][0])
    result['input_gradient'] = {k: dict(median_us=v[0], min_us=v[1], max_us=v[2]) for k, v in tb.items()}
    result['input_gradient'].update(samples=M, dy_dx_route_extra_us=round(route, 1), new_over_route=round(tb['grid_input_gradient'][0] / route, 3),
                                    new_over_forward=round(tb['grid_input_gradient'][0] / tb['forward'][0], 3),
                                    dy_dx_bytes_written_and_read=2 * M * L * 3 * 2 * 2)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
