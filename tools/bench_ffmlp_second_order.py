"""Cost of the FFMLP's second-order backward at the config-4 shape (main_sdf.py --fp16 --ff: hash grid L16 F2 T2^19, 16 -> 2048, feeding
FFMLP 32 -> 64 x 3 -> 1 softplus, 2^18 points, autocast): the median time of the first backward (ngp_ffmlp_backward with the input gradient,
what _ffmlp_forward.backward issues), of the double backward (ngp_ffmlp_backward_backward: d/d upstream gradient, d/d weights, d/d inputs,
workspace allocation included as in the op) and of whole eikonal training steps -- the FFMLP and, on the same box, the
Linear-Softplus-Linear stand-in DESIGN.md 3.6 was measured with -- from HIP events after warm-up.  One JSON line.

    python tools/bench_ffmlp_second_order.py [--points 262144] [--iters 50] [--warmup 10]
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

    from ffmlp import FFMLP
    from ffmlp import ffmlp as ff
    from gridencoder import GridEncoder
    dev = torch.device('cuda')
    din, hid, nl, act = 32, 64, 3, 5
    B = args.points
    assert B % 128 == 0
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {'shape': f'grid L16 C2 T2^19 16->2048 + FFMLP {din}->{hid}x{nl}->1 softplus', 'points': B, 'iters': args.iters}

    # the two entries alone, on the tensors the op hands them
    net = FFMLP(din, 1, hid, nl, activation='softplus').to(dev)
    w = net.weights.detach().half()
    x = (torch.rand(B, din, device=dev, generator=gen) - 0.5).half()
    g = torch.zeros(B, 16, device=dev, dtype=torch.half)
    g[:, 0] = 1.0
    u = ((torch.rand(B, din, device=dev, generator=gen) - 0.5) / 64).half()
    out = torch.empty(B, 16, device=dev, dtype=torch.half)
    fb = torch.empty(nl, B, hid, device=dev, dtype=torch.half)
    ff._backend.ffmlp_forward(x, w, B, din, 16, hid, nl, act, 6, fb, out)
    net_args = (din, 16, hid, nl, act, 6, True)
    d_w, d_x = torch.empty_like(w), torch.empty_like(x)
    result['first_backward_us'] = round(_median_us(lambda: ff._first_order_backward(g, x, w, fb, net_args), args.iters, args.warmup), 1)
    result['double_backward_us'] = round(_median_us(
        lambda: ff.ffmlp_backward_backward(g, x, w, fb, u, B, din, 16, hid, nl, act, None, d_w, d_x), args.iters, args.warmup), 1)

    # whole eikonal training steps: |sdf - gt| + 0.1 (|grad_x sdf| - 1)^2 through create_graph=True, under autocast
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048).to(dev)
    stand_in = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Softplus(), torch.nn.Linear(64, 64), torch.nn.Softplus(),
                                   torch.nn.Linear(64, 1)).to(dev)
    pts = torch.rand(B - 128, 3, device=dev, generator=gen) * 2 - 1   # (the module pads to the next multiple of 128: B rows in the kernels)
    gt = pts.norm(dim=-1) - 0.5

    def step(mlp):
        p = pts.detach().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.float16):
            sdf = mlp(enc(p))[:, 0].float()
            loss = (sdf - gt).abs().mean()
            grad_x = torch.autograd.grad(sdf.sum(), p, create_graph=True)[0]
            loss = loss + 0.1 * ((grad_x.norm(dim=-1) - 1.0) ** 2).mean()
        loss.backward()
        enc.embeddings.grad = None
        for q in mlp.parameters():
            q.grad = None

    result['eikonal_step_ffmlp_us'] = round(_median_us(lambda: step(net), args.iters, args.warmup), 1)
    result['eikonal_step_linear_stand_in_us'] = round(_median_us(lambda: step(stand_in), args.iters, args.warmup), 1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
