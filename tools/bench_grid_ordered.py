"""Cost of the ordered (bit-reproducible) scatter of the grid encoder's table gradient (csrc/grid_ordered.hip) beside the
atomic scatter it replaces, at the config-4 shape of DESIGN.md 3.6 (hash grid L16 F2 T2^19, 16 -> 2048, 2^18 random points): the first
backward with the input gradient for fp32 tables, and the double backward's u-terms for fp16 and fp32 tables, each on the atomic entry and
on the ordered one -- the median of `--iters` calls from HIP events after warm-up, the table zeroing included, in one process on one
device.  Also the fp16 first backward on its own record-sort path (with the three atomic figures: the four yardstick figures of DESIGN.md
3.6, measured in the same run) and the ordered workspace in bytes.  One JSON line.

    python tools/bench_grid_ordered.py [--points 262144] [--iters 50] [--warmup 10]
    python tools/bench_grid_ordered.py --one-cell      every point in ONE cell (runs of 2^18 records per corner and level): ONE timed call
                                                       per path after a warm-up on a small batch; run it under a time limit of its own
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


def _times_us(fn, iters, warmup):
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
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1 << 18)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--one-cell', action='store_true')
    args = ap.parse_args()

    import _ngp_capi as capi
    from gridencoder import backend, grid
    _backend = backend._backend
    dev = torch.device('cuda')
    D, C, L, H, log2_T = 3, 2, 16, 16, 19
    per_level_scale = float(np.exp2(np.log2(2048 / H) / (L - 1)))
    S = float(np.log2(per_level_scale))
    offsets = torch.from_numpy(grid.level_offsets(D, L, per_level_scale, H, log2_T, False)).to(dev)
    n = int(offsets[-1])
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {'shape': f'D{D} L{L} C{C} T2^{log2_T} H{H}->2048', 'points': args.points, 'one_cell': args.one_cell,
              'iters': 1 if args.one_cell else args.iters}

    def calls(B, dtype):
        """(first atomic, first ordered, second atomic, second ordered) on fresh inputs of B points"""
        if args.one_cell:
            x = (torch.full((B, D), 0.4321, device=dev) + 1e-6 * torch.rand(B, D, device=dev, generator=gen)).contiguous()
        else:
            x = torch.rand(B, D, device=dev, generator=gen)
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

        def first(fn):
            def run():
                gE.zero_()
                fn(g, x, E, offsets, gE, B, D, C, L, S, H, dy_dx, gx, 0, False, 0)
            return run

        def second(fn):
            def run():
                gE.zero_()
                fn(g, x, E, offsets, u, dg, gE, dx, B, D, C, L, S, H, 0, False, 0)
            return run

        return (first(_backend.grid_encode_backward), first(backend.grid_encode_backward_ordered),
                second(grid.grid_encode_backward_backward), second(backend.grid_encode_backward_backward_ordered))

    names = ('first_backward_atomic', 'first_backward_ordered', 'double_backward_atomic', 'double_backward_ordered')
    for tag, dtype in (('fp16', torch.float16), ('fp32', torch.float32)):
        if args.one_cell:
            for fn in calls(1024, dtype):   # code loading and allocator warm-up, not the timed shape
                fn()
            torch.cuda.synchronize()
        for name, fn in zip(names, calls(args.points, dtype)):
            if tag == 'fp16' and name.startswith('first'):
                # the fp16 first backward at this shape is on the record-sort path already (scatter_path 'sorted'): the existing entry alone,
                # the first of DESIGN.md 3.6's four yardstick figures (the others are the three atomic figures below)
                if name.endswith('ordered'):
                    continue
                name = 'first_backward_sorted'
            times = _times_us(fn, 1, 0) if args.one_cell else _times_us(fn, args.iters, args.warmup)
            result[f'{tag}_{name}_us'] = round(statistics.median(times), 1)
    result['ordered_workspace_bytes'] = int(capi.lib.ngp_grid_ordered_workspace_bytes(args.points, D, C, capi.NGP_F32))
    result['fp16_first_backward_path'] = backend.scatter_path(args.points, D, C, L, S, H, 0, False, torch.float16, True, 1, offsets)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
