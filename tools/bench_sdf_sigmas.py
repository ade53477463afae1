"""Cost of raymarching.sdf_sigmas (csrc/sdf_sigmas.hip: k_sdf_sigmas_fwd / _bwd / _inv_s) at the headline step's sample
count, M = 262 144 rows in fp32: forward + backward of
  the op            one launch forward, two backward (the row kernel and the one-workgroup pass that finishes grad_inv_s),
  the torch chain   the same definition as element-wise torch ops with their autograd (what a NeuS user writes without the op),
in the same process, timed alternately inside every repetition, HIP events around `batch` back-to-back forward + backward pairs, after
warm-up.  Also the bytes the op has to move (40 B per row forward; 44 B read + 28 B written backward, 40 B written with grad_dirs) over the
measured time, against which the launch path decides the cost at this size.  One JSON line.

    python tools/bench_sdf_sigmas.py [--rows 262144] [--inv-s 64] [--iters 100] [--warmup 10] [--batch 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

EPS, X_MAX = 1e-5, 15.0


def torch_chain(sdf, normals, dirs, deltas, inv_s, cos_anneal):
    """the op's definition in plain torch ops (tests/sdf_sigmas_cases.py: definition)"""
    d0 = deltas[:, 0]
    c = (dirs * normals).sum(-1)
    ic = -(F.relu(0.5 - 0.5 * c) * (1.0 - cos_anneal) + F.relu(-c) * cos_anneal)
    h = 0.5 * ic * d0
    x = torch.log(torch.sigmoid(inv_s * (sdf - h)) + EPS) - F.logsigmoid(inv_s * (sdf + h))
    live = d0 > 0
    return torch.where(live, torch.clamp(x, max=X_MAX) / torch.where(live, d0, torch.ones_like(d0)), torch.zeros_like(x))


def _time_us(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--inv-s', type=float, default=64.0)
    ap.add_argument('--cos-anneal', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=10)
    args = ap.parse_args()

    import raymarching
    from raymarching import backend as be
    dev = torch.device('cuda')
    gen = torch.Generator(device='cpu').manual_seed(0)
    M = args.rows
    rand = lambda *shape: torch.rand(*shape, generator=gen).to(dev)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    sdf = ((rand(M) * 0.2 - 0.1)).requires_grad_()
    normals = (unit(rand(M, 3) - 0.5) * (0.7 + 0.6 * rand(M, 1))).requires_grad_()
    dirs = unit(rand(M, 3) - 0.5)
    deltas = (rand(M, 2) * 0.045 + 0.005).contiguous()
    inv_s = torch.tensor([args.inv_s], device=dev, requires_grad=True)
    up = rand(M) - 0.5

    def run(op):
        def fn():
            sdf.grad = normals.grad = inv_s.grad = None
            op(sdf, normals, dirs, deltas, inv_s, args.cos_anneal).backward(up)
        return fn

    # the kernels alone (no autograd bookkeeping): the C entries on preallocated tensors
    sig, g_sdf, g_n, g_s = torch.empty(M, device=dev), torch.empty(M, device=dev), torch.empty(M, 3, device=dev), torch.empty(1, device=dev)
    sd, nd = sdf.detach(), normals.detach()
    s_det = inv_s.detach()

    def entries():
        be.sdf_sigmas_forward(sd, nd, dirs, deltas, s_det, M, args.cos_anneal, sig)
        be.sdf_sigmas_backward(up, sd, nd, dirs, deltas, s_det, M, args.cos_anneal, g_sdf, g_n, None, g_s)

    calls = {'op_fwd_bwd_us': run(raymarching.sdf_sigmas), 'entries_fwd_bwd_us': entries, 'torch_chain_fwd_bwd_us': run(torch_chain)}
    times = {k: [] for k in calls}
    for it in range(args.warmup + args.iters):
        for name, fn in calls.items():       # alternate the candidates inside every repetition
            us = _time_us(fn, args.batch)
            if it >= args.warmup:
                times[name].append(us)
    result = {'rows': M, 'inv_s': args.inv_s, 'iters': args.iters, 'batch': args.batch}
    result.update({k: round(statistics.median(v), 1) for k, v in times.items()})
    moved = M * (40 + 44 + 28)   # forward 36 B read + 4 B written; backward 44 B read + 28 B written (no grad_dirs here)
    result['bytes_moved'] = moved
    result['entries_gb_per_s'] = round(moved / (result['entries_fwd_bwd_us'] * 1e-6) / 1e9, 1)
    result['torch_chain_over_op'] = round(result['torch_chain_fwd_bwd_us'] / result['op_fwd_bwd_us'], 2)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
