"""Every output bit of the grid encoder's bit-reproducible table gradients -- the fp64 backwards (csrc/fp64.hip) and the ordered fp32 / fp16
scatter (csrc/grid_ordered.hip), which share one record sort (csrc/grid_records.hip) -- for a same-box comparison of two builds of
libngp_hip.so.

    NGP_HIP_LIBRARY=<one build> python tools/grid_records_bits.py --out a.npz        (a fresh process per library)
    NGP_HIP_LIBRARY=<other build> python tools/grid_records_bits.py --out b.npz
    python tools/grid_records_bits.py --compare a.npz b.npz                            (no GPU; exit status 1 on any difference)

Covered, through _ngp_capi alone: ngp_grid_encode_backward_ws in fp64 with and without dy_dx, ngp_grid_encode_backward_backward in fp64,
ngp_grid_encode_backward_ordered and ngp_grid_encode_backward_backward_ordered in fp32 and fp16.  General random inputs: a hand-made hashed
table with levels of 200, 4096 and 70000 entries (one, two and three 8-bit digits of the sort) at D = 3, C = 2, 4133 points, about 3 % of
them outside [0,1]^D and 500 within 2^-12 of one point (long runs); (D, C) = (2, 1), (4, 4), (5, 8) on the tests' general table; 40000
points at D = 3 (320000 records: two tiles per workgroup of a radix pass); bound = 2 on the ordered first order.  The whole table gradient is stored, accumulated onto nonzero
values, with every other output; outputs an entry must write are NaN-filled first.  The comparison is on the bytes."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), os.path.join(ROOT, 'tests'), ROOT]


def input_sets():
    """[(name, table dict of tests/grid_ordered_cases.py, B)]"""
    import grid_ordered_cases as goc
    digits = dict(name='digits', offs=np.array([0, 200, 4296, 74296], np.int32), S=1.0, H=16, D=3, L=3, C=2, gridtype=0, align=False, interp=0)
    sets = [('digits', digits, 4133)]
    for i, (D, C) in enumerate(((2, 1), (4, 4), (5, 8))):
        sets.append((f'general{D}x{C}', goc.general_table(D, C, gridtype=i % 2, align=i == 1, interp=i % 2), 1031))
    sets.append(('tiles2', goc.general_table(3, 2), 40000))
    return sets


def run(out_path):
    import torch
    import _ngp_capi as capi
    lib = capi.lib
    saved = {}
    dtypes = {'fp64': (torch.float64, capi.NGP_F64), 'fp32': (torch.float32, capi.NGP_F32), 'fp16': (torch.float16, capi.NGP_F16)}

    def keep(case, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            assert f'{case}/{name}' not in saved
            saved[f'{case}/{name}'] = t.detach().cpu().numpy()

    def scratch(nbytes):
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device='cuda'), int(nbytes)

    for name, tab, B in input_sets():
        gen = torch.Generator().manual_seed(31 + B + 7 * tab['D'] + tab['C'])
        D, C, L, n = tab['D'], tab['C'], tab['L'], int(tab['offs'][-1])
        level_args = (B, D, C, L, float(tab['S']), tab['H'])
        modes = (tab['gridtype'], int(tab['align']), tab['interp'])
        x = torch.rand(B, D, generator=gen)
        x[100:600] = 0.4 + torch.rand(D, generator=gen) * 2.0 ** -8 + torch.rand(500, D, generator=gen) * 2.0 ** -12   # one cell: long runs
        x[0], x[1] = 0.0, 1.0
        x[2::37, 0] = 1.0 + 2.0 ** -20                    # about 3 % outside, on either side
        x[5::71, D - 1] = -2.0 ** -24
        offs = torch.from_numpy(np.array(tab['offs'], np.int32)).cuda()
        base = dict(g=torch.randn(L, B, C, generator=gen), u=torch.randn(B, D, generator=gen), E=torch.rand(n, C, generator=gen) - 0.5,
                    init=torch.randn(n, C, generator=gen), dy_dx=torch.randn(B, L * D * C, generator=gen))
        for kind, (dtype, code) in dtypes.items():
            t = {k: v.to(dtype).cuda() for k, v in base.items()}
            xt = x.cuda()
            nan = lambda *shape: torch.full(shape, float('nan'), dtype=dtype, device='cuda')
            if kind == 'fp64':
                ws, nbytes = scratch(lib.ngp_grid_backward_workspace_bytes(None, *level_args, modes[0], modes[1], code))
                for with_inputs in (False, True):
                    ge, gi = t['init'].clone(), nan(B, D) if with_inputs else None
                    capi.check(lib.ngp_grid_encode_backward_ws(capi.ptr(t['g']), capi.ptr(xt), capi.ptr(t['E']), capi.ptr(offs), capi.ptr(ge), *level_args,
                                                               capi.ptr(t['dy_dx']) if with_inputs else None, capi.ptr(gi), *modes, code, 0.0, None,
                                                               capi.ptr(ws), nbytes, capi.stream()))
                    keep(f'{name}/fp64/first/inputs={with_inputs}', grad_embeddings=ge, **({'grad_inputs': gi} if with_inputs else {}))
                ws, nbytes = scratch(lib.ngp_grid_backward_backward_workspace_bytes(None, B, D, C, L, code))
                ge, gg, gx = t['init'].clone(), nan(L, B, C), nan(B, D)
                capi.check(lib.ngp_grid_encode_backward_backward(capi.ptr(t['g']), capi.ptr(xt), capi.ptr(t['E']), capi.ptr(offs), capi.ptr(t['u']),
                                                                 capi.ptr(gg), capi.ptr(ge), capi.ptr(gx), *level_args, *modes, code, capi.ptr(ws), nbytes,
                                                                 capi.stream()))
                keep(f'{name}/fp64/second', grad_embeddings=ge, grad_grad=gg, grad_inputs2=gx)
                continue
            ws, nbytes = scratch(lib.ngp_grid_ordered_workspace_bytes(B, D, C, code))
            # (bound = 2: the inputs are the same points spread over [-2, 2]; the fused mapping provides no grad_inputs)
            for bound in (0.0,) + ((2.0,) if name == 'digits' else ()):
                ge, gi = t['init'].clone(), None if bound else nan(B, D)
                xin = (xt * 4.0 - 2.0) if bound else xt
                capi.check(lib.ngp_grid_encode_backward_ordered(capi.ptr(t['g']), capi.ptr(xin), capi.ptr(t['E']), capi.ptr(offs), capi.ptr(ge), *level_args,
                                                                None if bound else capi.ptr(t['dy_dx']), capi.ptr(gi), *modes, code, bound, capi.ptr(ws),
                                                                nbytes, capi.stream()))
                keep(f'{name}/{kind}/ordered_first/bound={bound}', grad_embeddings=ge, **({} if bound else {'grad_inputs': gi}))
            ge, gg, gx = t['init'].clone(), nan(L, B, C), nan(B, D)
            capi.check(lib.ngp_grid_encode_backward_backward_ordered(capi.ptr(t['g']), capi.ptr(xt), capi.ptr(t['E']), capi.ptr(offs), capi.ptr(t['u']),
                                                                     capi.ptr(gg), capi.ptr(ge), capi.ptr(gx), *level_args, *modes, code, capi.ptr(ws),
                                                                     nbytes, capi.stream()))
            keep(f'{name}/{kind}/ordered_second', grad_embeddings=ge, grad_grad=gg, grad_inputs2=gx)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **saved)
    finite = sum(int(np.isfinite(a.astype(np.float64)).sum()) for a in saved.values())
    total = sum(a.size for a in saved.values())
    print(f'{capi.LIB_PATH}: {len(saved)} arrays, {sum(a.nbytes for a in saved.values())} bytes, {finite} of {total} values finite -> {out_path}')


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
    print(f'{len(a.files)} arrays compared, {sum(a[k].nbytes for k in a.files)} bytes, {bad} differ')
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
