"""Cost of the grid encoder's second-order backward at the config-4 shape (main_sdf.py: hash grid L16 F2 T2^19, 16 -> 2048, 2^18 points):
the median time of the first backward (ngp_grid_encode_backward_ws with the input gradient, what _grid_encode.backward issues) and of the
double backward's u-terms (ngp_grid_encode_backward_backward: d/d table, d/d upstream gradient, d/d inputs), fp16 tables (what autocast
makes) and fp32 tables, and of whole SDF training steps with and without the eikonal term, from HIP events after warm-up.  One JSON line.

    python tools/bench_grid_second_order.py [--points 262144] [--iters 50] [--warmup 10]
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


def _median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1 << 18)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()

    from gridencoder import grid
    from gridencoder.backend import _backend
    dev = torch.device('cuda')
    D, C, L, H, log2_T = 3, 2, 16, 16, 19
    per_level_scale = float(np.exp2(np.log2(2048 / H) / (L - 1)))
    S = float(np.log2(per_level_scale))
    offsets = torch.from_numpy(grid.level_offsets(D, L, per_level_scale, H, log2_T, False)).to(dev)
    n = int(offsets[-1])
    B = args.points
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, D, device=dev, generator=gen)
    result = {'shape': f'D{D} L{L} C{C} T2^{log2_T} H{H}->2048', 'points': B, 'iters': args.iters}
    for name, dtype in (('fp16', torch.float16), ('fp32', torch.float32)):
        E = ((torch.rand(n, C, device=dev, generator=gen) - 0.5) * 2e-2).to(dtype)
        g = (torch.rand(L, B, C, device=dev, generator=gen) - 0.5).to(dtype)
        u = (torch.rand(B, D, device=dev, generator=gen) - 0.5).to(dtype)
        out = torch.empty(L, B, C, device=dev, dtype=dtype)
        dy_dx = torch.empty(B, L * D * C, device=dev, dtype=dtype)
        _backend.grid_encode_forward(x, E, offsets, out, B, D, C, L, S, H, dy_dx, 0, False, 0)
        gE = torch.zeros_like(E)
        gx = torch.zeros(B, D, device=dev, dtype=dtype)
        dg = torch.empty(L, B, C, device=dev, dtype=dtype)
        dx = torch.empty(B, D, device=dev, dtype=dtype)

        def first():
            gE.zero_()
            _backend.grid_encode_backward(g, x, E, offsets, gE, B, D, C, L, S, H, dy_dx, gx, 0, False, 0)

        def second():
            gE.zero_()
            grid.grid_encode_backward_backward(g, x, E, offsets, u, dg, gE, dx, B, D, C, L, S, H, 0, False, 0)

        result[f'{name}_first_backward_us'] = round(_median_us(first, args.iters, args.warmup), 1)
        result[f'{name}_double_backward_us'] = round(_median_us(second, args.iters, args.warmup), 1)
        zero = _median_us(lambda: gE.zero_(), args.iters, args.warmup)
        result[f'{name}_table_zero_us'] = round(zero, 1)   # (included in both numbers above)
    # whole training steps of an SDF model (config-4 encoder + Linear(32,64)-Softplus-Linear(64,64)-Softplus-Linear(64,1)): the first-order
    # loss |sdf - gt| alone, and with the eikonal term 0.1 (|grad_x sdf| - 1)^2 through create_graph=True
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=D, num_levels=L, level_dim=C, base_resolution=H, log2_hashmap_size=log2_T, desired_resolution=2048).to(dev)
    mlp = torch.nn.Sequential(torch.nn.Linear(L * C, 64), torch.nn.Softplus(), torch.nn.Linear(64, 64), torch.nn.Softplus(),
                              torch.nn.Linear(64, 1)).to(dev)
    pts = torch.rand(B, D, device=dev, generator=gen) * 2 - 1
    gt = pts.norm(dim=-1) - 0.5

    def step(eikonal, autocast):
        x = pts.detach().requires_grad_(eikonal)
        with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
            sdf = mlp(enc(x))[:, 0].float()
            loss = (sdf - gt).abs().mean()
            if eikonal:
                grad_x = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
                loss = loss + 0.1 * ((grad_x.norm(dim=-1) - 1.0) ** 2).mean()
        loss.backward()
        enc.embeddings.grad = None
        for q in mlp.parameters():
            q.grad = None

    for name, autocast in (('fp16', True), ('fp32', False)):
        result[f'{name}_sdf_step_first_order_us'] = round(_median_us(lambda: step(False, autocast), args.iters, args.warmup), 1)
        result[f'{name}_sdf_step_eikonal_us'] = round(_median_us(lambda: step(True, autocast), args.iters, args.warmup), 1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
