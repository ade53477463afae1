"""Cost of the frequency and SH encoders' second-order backward (csrc/encoder_second.hip) at 2^18 points in fp32: the median
time of the first backward (what FrequencyEncoding.backward / _sh_encoder.backward issue) and of the double backward (one call of
ngp_freq_encode_backward_backward / ngp_sh_encode_backward_backward with both outputs) for the frequency encoder at D=3, deg=4 and
deg=10 and the SH encoder at degree 4 and 8, each with its algorithmic bytes per point and the bandwidth they imply; and of one eager SDF
step on FreqEncoder(3, 6) + Linear(39,64)-Softplus-Linear(64,64)-Softplus-Linear(64,1), with and without the eikonal term.  HIP events
after warm-up.  One JSON line.

    python tools/bench_encoder_second_order.py [--points 262144] [--iters 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

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

    import freqencoder.freq as fq
    import shencoder.sphere_harmonics as sh
    dev = torch.device('cuda')
    B = args.points
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen) * 2 - 1
    result = {'points': B, 'iters': args.iters}

    def record(name, first, second, bytes_first, bytes_second):
        for kind, fn, nbytes in (('first_backward', first, bytes_first), ('double_backward', second, bytes_second)):
            us = _median_us(fn, args.iters, args.warmup)
            result[f'{name}_{kind}_us'] = round(us, 1)
            result[f'{name}_{kind}_bytes_per_point'] = nbytes
            result[f'{name}_{kind}_GBps'] = round(nbytes * B / us / 1e3, 1)

    D = 3
    for deg in (4, 10):
        C = D * (1 + 2 * deg)
        x, g, u = rand(B, D), rand(B, C), rand(B, D)
        o = torch.empty(B, C, device=dev)
        fq._backend.freq_encode_forward(x, B, D, deg, C, o)
        gx, dg, dx = torch.empty(B, D, device=dev), torch.empty(B, C, device=dev), torch.empty(B, D, device=dev)
        record(f'freq_deg{deg}',
               lambda: fq._backend.freq_encode_backward(g, o, B, D, deg, C, gx),
               lambda: fq.freq_encode_backward_backward(g, o, u, B, D, deg, C, dg, dx),
               4 * (2 * C + D), 4 * (3 * C + 2 * D))
    for degree in (4, 8):
        N = degree * degree
        v = rand(B, 3)
        x, g, u = v / v.norm(dim=-1, keepdim=True), rand(B, N), rand(B, 3)
        y, dy_dx = torch.empty(B, N, device=dev), torch.empty(B, 3 * N, device=dev)
        sh._backend.sh_encode_forward(x, y, B, 3, degree, dy_dx)
        gx, dg, dx = torch.zeros(B, 3, device=dev), torch.empty(B, N, device=dev), torch.empty(B, 3, device=dev)
        # first: g and dy_dx read, grad_inputs read and written; double: dy_dx and u read, dL/dg written + g, x, u read, dL/dx written
        record(f'sh_degree{degree}',
               lambda: sh._backend.sh_encode_backward(g, x, B, 3, degree, dy_dx, gx),
               lambda: sh.sh_encode_backward_backward(g, x, dy_dx, u, B, 3, degree, dg, dx),
               4 * (4 * N + 6), 4 * (5 * N + 12))

    # one eager SDF step: |sdf - gt| alone, and with the eikonal term 0.1 (|grad_x sdf| - 1)^2 through create_graph=True
    enc = fq.FreqEncoder(3, 6)
    mlp = torch.nn.Sequential(torch.nn.Linear(enc.output_dim, 64), torch.nn.Softplus(), torch.nn.Linear(64, 64), torch.nn.Softplus(),
                              torch.nn.Linear(64, 1)).to(dev)
    pts = rand(B, 3)
    gt = pts.norm(dim=-1) - 0.5

    def step(eikonal):
        x = pts.detach().requires_grad_(eikonal)
        sdf = mlp(enc(x))[:, 0]
        loss = (sdf - gt).abs().mean()
        if eikonal:
            grad_x = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
            loss = loss + 0.1 * ((grad_x.norm(dim=-1) - 1.0) ** 2).mean()
        loss.backward()
        for q in mlp.parameters():
            q.grad = None

    result['freq_deg6_sdf_step_first_order_us'] = round(_median_us(lambda: step(False), args.iters, args.warmup), 1)
    result['freq_deg6_sdf_step_eikonal_us'] = round(_median_us(lambda: step(True), args.iters, args.warmup), 1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
