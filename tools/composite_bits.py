"""Every output bit of the training compositor's C entries on the ray table of tests/composite_geo_cases.py, for a same-box comparison of two
builds of libngp_hip.so (csrc/raymarching.hip: k_composite_train_fwd / _bwd / _geo_fwd / _geo_bwd / _loss_bwd / _geo_loss_bwd; csrc/fp64.hip:
their float64 twins).

    NGP_HIP_LIBRARY=<one build> python tools/composite_bits.py --out a.npz      (a fresh process per library)
    NGP_HIP_LIBRARY=<other build> python tools/composite_bits.py --out b.npz
    python tools/composite_bits.py --compare a.npz b.npz                          (no GPU; exit status 1 on any difference)

N = 10, M = 1600 (empty, 1, 63, 64, 65, 130 and 300 samples, saturating inside the first row, T_thresh crossed at the row boundary, an
overflowing ray, shuffled output rows), both `early` variants, the per-ray inputs of tests/test_gpu_fused_geo_loss.py and the upstream
gradients of composite_geo_cases.upstream().  Every output buffer is NaN-filled before the call -- zero-filled where the entry's contract has
the caller pre-zero it -- and stored whole, so a row that a build must not touch is compared too.  The comparison is on the bytes."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), os.path.join(ROOT, 'tests'), ROOT]


def run(out_path):
    import torch
    import _ngp_capi as capi
    import composite_geo_cases as C
    import test_gpu_fused_geo_loss as F   # its seeded inputs: nears, fars, target, bg, target depth, depth weights
    lib, st = capi.lib, capi.stream()
    N, M, T = F.N, C.M, C.T_THRESH
    P = capi.ptr
    saved = {}

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float('nan'), device='cuda', dtype=dtype)

    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, device='cuda', dtype=dtype)

    def keep(case, **arrays):
        torch.cuda.synchronize()
        for name, t in arrays.items():
            assert f'{case}/{name}' not in saved
            saved[f'{case}/{name}'] = t.cpu().numpy()

    for early in (True, False):
        i = F._inputs(early)
        up = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in C.upstream().items()}
        used = torch.tensor([i['used']], dtype=torch.int32, device='cuda')
        tag = f'early={early}'
        common = (P(i['sigma']), P(i['rgb']), P(i['deltas']), P(i['rays']))

        # ---- the stand-alone plain entries ----
        fwd = {}
        for bg_mode in (0, 1, 2):
            o = dict(weights_sum=nan(N), depth=nan(N), image=nan(N, 3), image_out=nan(N, 3), depth_out=nan(N))
            capi.check(lib.ngp_composite_rays_train_forward_ex(*common, M, N, T, P(o['weights_sum']), P(o['depth']), P(o['image']), bg_mode, F.BG_SCALAR,
                                                               P(i['bg']) if bg_mode == 2 else None, P(i['nears']), P(i['fars']), P(o['image_out']),
                                                               P(o['depth_out']), st))
            keep(f'{tag}/forward_ex/bg={bg_mode}', **o)
            fwd = o
        for bg_mode, with_rows, with_gw in itertools.product((0, 1, 2), (True, False), (True, False)):
            if bg_mode == 0 and not with_gw:
                continue   # the entry refuses it
            fill = nan if with_rows else zeros   # rows_used: the outputs arrive uninitialised; NULL: the caller pre-zeroes
            o = dict(grad_sigmas=fill(M), grad_rgbs=fill(M, 3))
            capi.check(lib.ngp_composite_rays_train_backward_ex(P(up['weights_sum']) if with_gw else None, P(up['image']), *common, P(fwd['weights_sum']),
                                                                P(fwd['image']), M, N, T, P(o['grad_sigmas']), P(o['grad_rgbs']), bg_mode, F.BG_SCALAR,
                                                                P(i['bg']) if bg_mode == 2 else None, P(used) if with_rows else None, st))
            keep(f'{tag}/backward_ex/bg={bg_mode},rows_used={with_rows},grad_ws={with_gw}', **o)

        # ---- the stand-alone geometry entries ----
        g = dict(weights_sum=nan(N), depth=nan(N), image=nan(N, 3), distortion=nan(N))
        capi.check(lib.ngp_composite_rays_train_geo_forward(*common, M, N, T, P(g['weights_sum']), P(g['depth']), P(g['image']), P(g['distortion']), st))
        keep(f'{tag}/geo_forward', **g)
        for given in (('weights_sum', 'depth', 'image', 'distortion'), ('weights_sum', 'image'), ('depth',), ('distortion',)):
            o = dict(grad_sigmas=zeros(M), grad_rgbs=zeros(M, 3))
            gp = {k: P(up[k]) if k in given else None for k in up}
            capi.check(lib.ngp_composite_rays_train_geo_backward(gp['weights_sum'], gp['depth'], gp['image'], gp['distortion'], *common, P(g['weights_sum']),
                                                                 P(g['depth']), P(g['image']), P(g['distortion']), M, N, T, P(o['grad_sigmas']),
                                                                 P(o['grad_rgbs']), st))
            keep(f'{tag}/geo_backward/grads={"+".join(given)}', **o)

        # ---- the two one-launch training steps ----
        scale = torch.tensor([128.0], device='cuda')
        for bg_mode, with_loss, scaled in itertools.product((1, 2), (True, False), (True, False)):
            bg = P(i['bg']) if bg_mode == 2 else None
            ws = F._workspace(i)
            o = dict(weights_sum=nan(N), image=nan(N, 3), depth=nan(N), loss=nan(1), ray_err=nan(N), grad_sigmas=nan(M),
                     grad_out16=nan(M, 16, dtype=torch.half))
            capi.check(lib.ngp_composite_train_loss_backward(*common, M, N, T, bg_mode, F.BG_SCALAR, bg, P(i['nears']), P(i['fars']), P(i['target']),
                                                             P(scale) if scaled else None, P(o['weights_sum']), P(o['image']), P(o['depth']),
                                                             P(o['loss']) if with_loss else None, P(o['ray_err']), P(o['grad_sigmas']), P(o['grad_out16']),
                                                             P(ws), ws.numel() * 4, st))
            keep(f'{tag}/loss_backward/bg={bg_mode},loss={with_loss},scale={scaled}', workspace=ws, **o)
            for lam_dist, lam_depth in ((0.0, 0.0), (F.LAMBDA_DISTORTION, F.LAMBDA_DEPTH)):
                ws = F._workspace(i)
                o = dict(weights_sum=nan(N), image=nan(N, 3), depth=nan(N), depth_raw=nan(N), distortion=nan(N), loss=nan(1), ray_err=nan(N),
                         grad_sigmas=nan(M), grad_out16=nan(M, 16, dtype=torch.half))
                capi.check(lib.ngp_composite_train_geo_loss_backward(*common, M, N, T, bg_mode, F.BG_SCALAR, bg, P(i['nears']), P(i['fars']), P(i['target']),
                                                                     lam_dist, lam_depth, P(i['z']), P(i['m']), P(scale) if scaled else None,
                                                                     P(o['weights_sum']), P(o['image']), P(o['depth']), P(o['depth_raw']),
                                                                     P(o['distortion']), P(o['loss']) if with_loss else None, P(o['ray_err']),
                                                                     P(o['grad_sigmas']), P(o['grad_out16']), P(ws), ws.numel() * 4, st))
                keep(f'{tag}/geo_loss_backward/bg={bg_mode},loss={with_loss},scale={scaled},lambdas={lam_dist},{lam_depth}', workspace=ws, **o)

        # ---- float64: plain and geometry, forward and backward ----
        t = C.ray_table(early)
        d64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        s64, c64, dl64 = d64(t['sigmas']), d64(t['rgbs']), d64(t['deltas'])
        up64 = {k: d64(v) for k, v in C.upstream().items()}
        common64 = (P(s64), P(c64), P(dl64), P(i['rays']))
        f8 = torch.float64
        p = dict(weights_sum=nan(N, dtype=f8), depth=nan(N, dtype=f8), image=nan(N, 3, dtype=f8))
        capi.check(lib.ngp_composite_rays_train_forward_f64(*common64, M, N, T, P(p['weights_sum']), P(p['depth']), P(p['image']), st))
        keep(f'{tag}/forward_f64', **p)
        o = dict(grad_sigmas=zeros(M, dtype=f8), grad_rgbs=zeros(M, 3, dtype=f8))
        capi.check(lib.ngp_composite_rays_train_backward_f64(P(up64['weights_sum']), P(up64['image']), *common64, P(p['weights_sum']), P(p['image']), M, N, T,
                                                             P(o['grad_sigmas']), P(o['grad_rgbs']), st))
        keep(f'{tag}/backward_f64', **o)
        g = dict(weights_sum=nan(N, dtype=f8), depth=nan(N, dtype=f8), image=nan(N, 3, dtype=f8), distortion=nan(N, dtype=f8))
        capi.check(lib.ngp_composite_rays_train_geo_forward_f64(*common64, M, N, T, P(g['weights_sum']), P(g['depth']), P(g['image']), P(g['distortion']), st))
        keep(f'{tag}/geo_forward_f64', **g)
        for given in (('weights_sum', 'depth', 'image', 'distortion'), ('weights_sum', 'image')):
            o = dict(grad_sigmas=zeros(M, dtype=f8), grad_rgbs=zeros(M, 3, dtype=f8))
            gp = {k: P(up64[k]) if k in given else None for k in up64}
            capi.check(lib.ngp_composite_rays_train_geo_backward_f64(gp['weights_sum'], gp['depth'], gp['image'], gp['distortion'], *common64,
                                                                     P(g['weights_sum']), P(g['depth']), P(g['image']), P(g['distortion']), M, N, T,
                                                                     P(o['grad_sigmas']), P(o['grad_rgbs']), st))
            keep(f'{tag}/geo_backward_f64/grads={"+".join(given)}', **o)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **saved)
    finite = sum(int(np.isfinite(a.astype(np.float64)).sum()) for a in saved.values())
    print(f'{capi.LIB_PATH}: {len(saved)} arrays, {sum(a.nbytes for a in saved.values())} bytes, {finite} finite values -> {out_path}')


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    bad = 0
    for key in sorted(a.files):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8))
        if not same:
            bad += 1
            where = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))[:4] if x.shape == y.shape and x.dtype == y.dtype else None
            print(f'DIFFERENT {key}: {x.dtype}{x.shape} against {y.dtype}{y.shape}, first differing bytes {where}')
    print(f'{len(a.files)} arrays compared, {bad} differ')
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='run the entries of the selected library and store every output here (.npz)')
    ap.add_argument('--compare', nargs=2, metavar='NPZ', help='compare two stored runs byte for byte')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error('--out or --compare')
    run(args.out)
