"""Every output bit of the record-sort grid backward (csrc/gridencoder.hip) on the calls of tests/test_gpu_grid_backward_paths.py, for a
same-box comparison of two builds of libngp_hip.so.

    NGP_HIP_LIBRARY=<one build> python tools/grid_backward_bits.py --out a.npz        (a fresh process per library)
    NGP_HIP_LIBRARY=<other build> python tools/grid_backward_bits.py --out b.npz
    python tools/grid_backward_bits.py --compare a.npz b.npz                            (no GPU; exit status 1 on any difference)

Stored whole: the table gradient of every call (the six index modes on T1 / T2; the forwarding entries with and without found_inf and slab
sets, finite and with one infinite gradient; the overwriting call into a NaN-filled table; gradients x 6000; stale host offsets, both
kinds), found_inf where given, the carried slab outputs and the loss of one call that carries them, and for T1 and T3 the raw workspace
(descriptors and records) after the call.  The bytes of a workspace that the kernels never write (pair-unit areas behind a chunk's last
record, padding) are found by running the call twice with two different fill bytes: a byte that holds its fill both times is zeroed in
the stored copy, and the mask is stored too.  (tools/optim_bits.py covers the flush that carries the table's Adam sweep.)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

MODES = [(2, 0, False, 0), (2, 1, True, 1), (3, 1, False, 0), (3, 0, True, 0), (3, 0, False, 1), (3, 1, True, 1)]


def run(out_path):
    import torch
    import _ngp_capi as capi
    import grid_backward_path_cases as pc
    saved = {}

    def keep(case, out):
        saved[case + '/table'] = out['ge'].cpu().numpy()
        if out['found_inf'] is not None:
            saved[case + '/found_inf'] = out['found_inf'].cpu().numpy()

    def sets(**fields):
        s = capi.SlabSets()
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    for B in pc.BATCHES:
        for D, gridtype, align, interp in MODES:
            name = 'T1' if D == 3 else 'T2'
            x, g = pc.ray_inputs(name, B)
            keep(f'modes/{name},B={B},gridtype={gridtype},align={align},interp={interp}',
                 pc.run(pc.table(name, align), x, g, gridtype=gridtype, align=align, interp=interp))
        for name in ('T1', 'T2', 'T3'):
            tab = pc.table(name)
            x, g = pc.inputs(name, B)
            bad = np.array(g)
            bad[tab['L'] - 1, 77, 0] = np.inf
            for entry, found_inf, given in (('ws', False, None), ('checked', False, None), ('checked', True, None), ('slabs', False, None),
                                            ('slabs', True, None), ('slabs', False, sets()), ('slabs', True, sets())):
                keep(f'entries/{name},B={B},{entry},found_inf={found_inf},sets={given is not None}', pc.run(tab, x, g, entry=entry, found_inf=found_inf, sets=given))
            for entry in ('checked', 'slabs'):
                keep(f'entries/{name},B={B},{entry},inf', pc.run(tab, x, bad, entry=entry, found_inf=True))
            if name != 'T2':
                nan = torch.full((int(tab['offs'][-1]), 2), float('nan'), device='cuda', dtype=torch.half)
                keep(f'overwrite/{name},B={B}', pc.run(tab, x, g, entry='slabs', ge=nan, found_inf=True, sets=sets(overwrite_table=1)))
                # the raw workspace: two fills tell the bytes the kernels never write
                a, b = pc.run(tab, x, g, ws_fill=0xAB)['ws'].cpu().numpy(), pc.run(tab, x, g, ws_fill=0x54)['ws'].cpu().numpy()
                unwritten = (a == 0xAB) & (b == 0x54)
                assert np.array_equal(a[~unwritten], b[~unwritten]), 'the written bytes of the workspace differ between two calls'
                saved[f'workspace/{name},B={B}/bytes'] = np.where(unwritten, 0, a).astype(np.uint8)
                saved[f'workspace/{name},B={B}/unwritten'] = np.packbits(unwritten)
        tab = pc.table('T1')
        x, g = pc.ray_inputs('T1', B, magnitude=6000.0)
        keep(f'scaled/T1,B={B}', pc.run(tab, x, g, entry='checked', found_inf=True))
        x, g = pc.ray_inputs('T1', B)
        for size in (16384, 30000):
            dev = pc.resized(tab['offs'], 5, size)
            keep(f'stale/T1,B={B},level5={size},right', pc.run(tab, x, g, offs=dev))
            keep(f'stale/T1,B={B},level5={size},stale', pc.run(tab, x, g, offs=dev, host_offs=tab['offs']))
        x, g = pc.lattice_inputs('T1', B, 0)
        dev = pc.resized(tab['offs'], 0, pc.DENSE_BINS * pc.SLICE + 8)
        keep(f'stale/T1,B={B},level0=outgrown,right', pc.run(tab, x, g, offs=dev))
        keep(f'stale/T1,B={B},level0=outgrown,stale', pc.run(tab, x, g, offs=dev, host_offs=tab['offs']))
        # the carried reductions in the accumulate launch: two slab sets and the loss sum (NaN-filled outputs)
        gen = torch.Generator().manual_seed(B)
        for name in ('T1', 'T3'):
            tab = pc.table(name)
            x, g = pc.inputs(name, B)
            sl = [torch.randn(n, p, generator=gen).cuda() for n, p in ((5, 3072), (3, 1000))]
            gw = [torch.full((s.shape[1],), float('nan'), device='cuda', dtype=torch.half) for s in sl]
            err, loss = torch.rand(777, generator=gen).cuda(), torch.full((1,), float('nan'), device='cuda')
            s = sets(slabs_a=sl[0].data_ptr(), n_slabs_a=5, n_params_a=3072, grad_weights_a=gw[0].data_ptr(), slabs_b=sl[1].data_ptr(), n_slabs_b=3,
                     n_params_b=1000, grad_weights_b=gw[1].data_ptr(), ray_err=err.data_ptr(), n_rays=777, loss=loss.data_ptr())
            keep(f'carried/{name},B={B}', pc.run(tab, x, g, entry='slabs', found_inf=True, sets=s))
            saved[f'carried/{name},B={B}/grad_weights_a'], saved[f'carried/{name},B={B}/grad_weights_b'] = gw[0].cpu().numpy(), gw[1].cpu().numpy()
            saved[f'carried/{name},B={B}/loss'] = loss.cpu().numpy()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **saved)
    print(f'{capi.LIB_PATH}: {len(saved)} arrays, {sum(a.nbytes for a in saved.values())} bytes -> {out_path}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='run the calls under the selected library and store every output here (.npz)')
    ap.add_argument('--compare', nargs=2, metavar='NPZ', help='compare two stored runs byte for byte')
    args = ap.parse_args()
    if args.compare:
        from optim_bits import compare
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error('--out or --compare')
    run(args.out)
