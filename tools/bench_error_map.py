"""Cost of error-map ray sampling per training step (csrc/error_map.hip) at the reference recipe's shape: a 128 x 128 map,
N = 4096 rays, an 800 x 800 frame, one image per step.

  A  the torch path: get_rays(error_map=) -- torch.multinomial without replacement (exponential fill, divide, top-k), two torch.rand
     refinements, the rays kernel -- plus the Trainer's update in torch (per-ray mean squared error, gather, 0.1 / 0.9 EMA, scatter_);
  B  the native pair: get_rays(error_map=, seed=) -- ngp_error_map_draw, the rays kernel -- plus ErrorMaps.update (ngp_error_map_update).
Also the halves of each (draw + rays / update alone), and whether A can be captured into a HIP graph on this torch build at all (B can:
tests/test_gpu_error_map.py replays it).

A and B are timed alternately inside every repetition of one process, after a warm-up: device time from HIP events around `batch`
back-to-back calls, and host wall time around the same calls ending in a synchronise (what a training loop that waits for nothing else
would see; the torch path is a chain of small launches, so the two differ).  Medians over the repetitions with their spread (min .. max).
One JSON line.

    python tools/bench_error_map.py [--iters 60] [--warmup 10] [--batch 5]
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
    """(device us, host wall us) per call of `batch` back-to-back calls"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / batch
    return a.elapsed_time(b) * 1000.0 / batch, wall


def _alternate(fns, iters, warmup, batch):
    """{name: {'device_us': (median, min, max), 'wall_us': (...)}} of callables timed alternately"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    t = {k: ([], []) for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            d, w = _time_us(fn, batch)
            t[k][0].append(d)
            t[k][1].append(w)
    stat = lambda v: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1))
    return {k: {'device_us': stat(v[0]), 'wall_us': stat(v[1])} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--probe-capture', action='store_true', help='only try to capture the torch path into a graph and say what happened')
    args = ap.parse_args()
    assert args.iters >= 50, 'at least 50 repetitions'
    assert torch.cuda.is_available(), 'bench_error_map needs a GPU'
    from nerf import utils

    dev = torch.device('cuda')
    torch.manual_seed(0)
    res, N, H, W = args.res, args.rays, args.size, args.size
    maps = utils.ErrorMaps(4, dev, res=res)
    maps.maps.uniform_(0.01, 1.0)
    torch_maps = maps.maps.clone()
    poses = torch.eye(4, device=dev)[None].clone()
    poses[0, :3, 3] = torch.tensor([0.1, 0.2, 3.0], device=dev)
    intr = (1111.0, 1111.0, W / 2, H / 2)
    out = (torch.empty(1, N, 3, device=dev), torch.empty(1, N, 3, device=dev))
    image, target = torch.rand(N, 3, device=dev), torch.rand(N, 3, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    state = {}

    def a_draw():
        # (the reference hard-codes the 128 x 128 map; other --res values time the native side only)
        state['a'] = utils.get_rays(poses, intr, H, W, N, error_map=torch_maps[1:2], out=out)

    def a_update():
        coarse = state['a']['inds_coarse']
        error = ((image - target) ** 2).mean(-1)                      # Trainer.train_step: loss.mean(-1) before the reduction
        old = torch_maps[1:2].gather(1, coarse)
        torch_maps[1:2].scatter_(1, coarse, 0.1 * old + 0.9 * error[None])

    def b_draw():
        state['b'] = utils.get_rays(poses, intr, H, W, N, error_map=maps.maps[1:2], seed=step, out=out, res=res)

    def b_update():
        maps.update(1, state['b']['inds_coarse'][0], image, target)

    def a_step():
        a_draw()
        a_update()

    def b_step():
        b_draw()
        b_update()
        step.add_(1)      # (what the optimizer's step count does for free inside the training step; counted against B here)

    if args.probe_capture:
        a_step()
        torch.cuda.synchronize()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                a_step()
            g.replay()
            torch.cuda.synchronize()
            print('capture: captured and replayed')
        except Exception as e:  # noqa: BLE001 -- the answer is the error
            print('capture: refused: ' + ' '.join(repr(e).split())[:300])
        return

    a_draw()
    b_draw()
    fns = {'B native: draw + rays + update': b_step, 'B native: draw + rays': b_draw, 'B native: update': b_update}
    if res == 128:
        fns = {'A torch: draw + rays + update': a_step, 'A torch: draw + rays': a_draw, 'A torch: update': a_update, **fns}
    times = _alternate(fns, args.iters, args.warmup, args.batch)

    # can the torch path be captured at all?  Asked in a fresh child process: a refused capture leaves its process's stream state behind
    capture = None
    if res == 128:
        import subprocess
        torch.cuda.synchronize()
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--probe-capture'], capture_output=True, text=True, timeout=300)
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith('capture: ')]
        capture = lines[-1][len('capture: '):] if lines else f'probe ended with status {child.returncode}'
    result = {'bench': 'error_map', 'res': res, 'rays': N, 'frame': [H, W], 'iters': args.iters, 'warmup': args.warmup, 'batch': args.batch,
              'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'times': times, 'torch_path_graph_capture': capture}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
