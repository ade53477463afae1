"""Every output bit of the FFMLP backward's C entries, for a same-box comparison of two builds of libngp_hip.so (csrc/ffmlp.hip:
k_ffmlp_backward, k_ffmlp_backward_paired, the layered kernels' reduction, k_ffmlp_reduce_slabs_pair; csrc/gridencoder.hip: the reductions the
grid backward carries).

    NGP_HIP_LIBRARY=<one build> python tools/ffmlp_backward_bits.py --out a.npz      (a fresh process per library)
    NGP_HIP_LIBRARY=<other build> python tools/ffmlp_backward_bits.py --out b.npz
    python tools/ffmlp_backward_bits.py --compare a.npz b.npz                          (no GPU; exit status 1 on any difference)

Inputs: the recipe of tests/test_gpu_ffmlp_slab_sum.py::_case (output gradients scaled by 1024, so the fp32 partial sums round and a changed
order of additions shows).  grad_inputs and grad_weights start as NaN, backward_buffer as zero; every buffer is stored whole for B <= 2176,
as the SHA-256 of its bytes above.  Batches: 128 (one workgroup, direct fp16 store), 640 (five workgroups), 2176 (17 slabs on the 64-wide
nets of 2 and 3 layers: reduction group 0 adds two), 32896 (a second round of tiles in workgroup 0; paired 64-wide shapes only).
Register-resident shapes: hidden 32 / 64 x input_dim 16 / 32 / 48 / 64 x 2 / 3 / 4 layers -- every (WIDTH, IN_JB, NHM) of the dispatch --
with ReLU and sigmoid, with and without dL/dx, flags 0 / NGP_FF_SINGLE_WAVE / NGP_FF_SERIAL_FLUSH / NGP_FF_DEFER_REDUCE where the shape accepts
them, planar input and dL/dx, NGP_FF_RECOMPUTE where a recomputing kernel exists.  Layered shapes (32, 128, 2) and (32, 64, 6) with and
without a workspace, the colour entry, ngp_ffmlp_reduce_slabs_pair, and one ngp_grid_encode_backward_checked_slabs call that carries two slab
sets and the loss sum (with a workspace: inside the accumulate launch; without: on their own)."""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

WHOLE_UP_TO = 2176


def n_params(din, hid, nl):
    return hid * (din + hid * (nl - 1) + 16)


def run(out_path):
    import torch
    import _ngp_capi as capi
    import oracle
    lib, st, P = capi.lib, capi.stream(), capi.ptr
    SINGLE, SERIAL, DEFER, RECOMP = capi.NGP_FF_SINGLE_WAVE, capi.NGP_FF_SERIAL_FLUSH, capi.NGP_FF_DEFER_REDUCE, capi.NGP_FF_RECOMPUTE
    PLANAR = capi.NGP_FF_INPUT_PLANAR | capi.NGP_FF_DX_PLANAR
    saved = {}
    half = dict(device='cuda', dtype=torch.half)

    def keep(case, B, **arrays):
        torch.cuda.synchronize()
        for name, t in arrays.items():
            key = f'{case}/{name}'
            assert key not in saved, key
            a = np.ascontiguousarray(t.cpu().numpy())
            saved[key] = a if B <= WHOLE_UP_TO else np.frombuffer(hashlib.sha256(a.reshape(-1).view(np.uint8).tobytes()).digest(), dtype=np.uint8)

    def inputs(B, din, hid, nl, act, planar):
        g = torch.Generator(device='cuda').manual_seed(B + 7 * din + 11 * hid + 13 * nl)
        x = (torch.rand(B, din, device='cuda', generator=g) * 2 - 1).half()
        if planar:
            x = x.view(B, din // 2, 2).permute(1, 0, 2).contiguous()
        w = ((torch.rand(n_params(din, hid, nl), device='cuda', generator=g) * 2 - 1) * (3 / hid) ** 0.5).half()
        dy = torch.randn(B, 16, device='cuda', generator=g).half() * 1024   # an exact scaling
        fb = torch.empty(nl, B, hid, **half)
        out = torch.empty(B, 16, **half)
        capi.check(lib.ngp_ffmlp_forward_ex(P(x), P(w), B, din, 16, hid, nl, act, 6, P(fb), P(out), capi.NGP_FF_INPUT_PLANAR if planar else 0, st))
        return x, w, dy, fb

    def backward(case, B, din, hid, nl, act, flags, with_dx, data, workspace=False):
        x, w, dy, fb = data
        gi = torch.full((B * din,), float('nan'), **half)
        gw = torch.full((n_params(din, hid, nl),), float('nan'), **half)
        bb = torch.zeros(nl, B, hid, **half)
        nbytes = int(lib.ngp_ffmlp_backward_workspace_bytes(B, din, hid, nl)) if workspace else 0
        ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda') if nbytes else None
        capi.check(lib.ngp_ffmlp_backward_ws(P(dy), P(x), P(w), None if flags & RECOMP else P(fb), B, din, 16, hid, nl, act, 6, 1 if with_dx else 0,
                                             P(bb), P(gi), P(gw), flags, P(ws), nbytes, st))
        keep(case, B, grad_inputs=gi, grad_weights=gw, backward_buffer=bb)

    # ---- the register-resident shapes ----
    for hid, nl in ((64, 2), (64, 3)):   # the 17 slabs at 2176 are what the tool's cases are chosen for: asserted, not trusted
        assert lib.ngp_ffmlp_backward_slab_count(2176, 32, hid, nl) > 16, 'B = 2176 no longer leaves more than 16 slabs'
    for hid, din, nl, act in itertools.product((32, 64), (16, 32, 48, 64), (2, 3, 4), (0, 3)):
        batches = (128, 640, 2176) + ((32896,) if hid == 64 and nl <= 3 else ())
        for B in batches:
            tag = f'ffmlp/hid={hid},in={din},nl={nl},act={act},B={B}'
            data = inputs(B, din, hid, nl, act, False)
            flag_sets = [0, SINGLE, SERIAL] + ([DEFER] if nl <= 3 else [])
            for flags in flag_sets:
                backward(f'{tag}/flags={flags},dx=1', B, din, hid, nl, act, flags, True, data)
            for flags in [0] + ([DEFER] if nl <= 3 else []):
                backward(f'{tag}/flags={flags},dx=0', B, din, hid, nl, act, flags, False, data)
            recompute = hid == 64 and din == 32 and nl <= 3 and act == 0
            if recompute:
                for flags in (RECOMP, RECOMP | DEFER, RECOMP | SERIAL):
                    backward(f'{tag}/flags={flags},dx=1', B, din, hid, nl, act, flags, True, data)
            data = inputs(B, din, hid, nl, act, True)
            for flags in [PLANAR] + ([PLANAR | RECOMP] if recompute else []):
                backward(f'{tag}/flags={flags},dx=1', B, din, hid, nl, act, flags, True, data)

    # ---- the layered shapes: the fourth launch site of the reduction ----
    for (din, hid, nl), B, workspace in itertools.product(((32, 128, 2), (32, 64, 6)), (640, 2176), (True, False)):
        data = inputs(B, din, hid, nl, 0, False)
        backward(f'layered/hid={hid},in={din},nl={nl},B={B},workspace={workspace}', B, din, hid, nl, 0, 0, True, data, workspace=workspace)

    # ---- the colour entry of the fused network ----
    for nl, B in itertools.product((2, 3), (128, 640, 2176, 32896)):
        x, w, dy, fb = inputs(B, 32, 64, nl, 0, False)
        g = torch.Generator(device='cuda').manual_seed(B + nl)
        h16 = torch.randn(B, 16, device='cuda', generator=g).half()
        g_sigma = torch.randn(B, device='cuda', generator=g) * 0.01
        for flags in (0, DEFER, RECOMP, SERIAL, DEFER | RECOMP):
            g_h16 = torch.full((B, 16), float('nan'), **half)
            gw = torch.full_like(w, float('nan'))
            bb = torch.zeros(nl, B, 64, **half)
            capi.check(lib.ngp_network_backward_color(P(dy), P(x), P(w), None if flags & RECOMP else P(fb), B, nl, P(bb), P(g_sigma), P(h16), 1.3,
                                                      P(g_h16), P(gw), flags, st))
            keep(f'color/nl={nl},B={B},flags={flags}', B, grad_h16=g_h16, grad_w_color=gw, backward_buffer=bb)

    # ---- the pair reduction; the same sets carried by the grid backward (tests/test_gpu_pipeline.py) ----
    g = torch.Generator(device='cuda').manual_seed(77)
    n_a, n_b, s_a, s_b = 64 * (32 + 64 + 16), 64 * (32 + 128 + 16), 37, 5
    slabs_a, slabs_b = torch.randn(s_a, n_a, device='cuda', generator=g), torch.randn(s_b, n_b, device='cuda', generator=g)
    direct_a, direct_b = torch.randn(n_a, device='cuda', generator=g).half(), torch.randn(n_b, device='cuda', generator=g).half()
    for inf, with_found, (use_a, use_b) in itertools.product((False, True), (True, False), ((True, True), (True, False), (False, True))):
        sb = slabs_b.clone()
        if inf:
            sb[3, 100] = float('inf')
        # a set without slabs holds gradients its backward stored directly: only swept for found_inf
        gw_a = torch.full((n_a,), float('nan'), **half) if use_a else direct_a.clone()
        gw_b = torch.full((n_b,), float('nan'), **half) if use_b else direct_b.clone()
        found = torch.zeros(1, device='cuda')
        capi.check(lib.ngp_ffmlp_reduce_slabs_pair(P(slabs_a) if use_a else None, s_a if use_a else 0, n_a, P(gw_a), P(sb) if use_b else None,
                                                   s_b if use_b else 0, n_b, P(gw_b), P(found) if with_found else None, st))
        keep(f'pair/inf={inf},found_inf={with_found},a={use_a},b={use_b}', 0, grad_weights_a=gw_a, grad_weights_b=gw_b, found_inf=found)

    M = 1 << 15
    offs, pls = oracle.grid_offsets(desired_resolution=2048)
    S, toffs = float(np.log2(pls)), torch.from_numpy(offs).cuda()
    x = torch.rand(M, 3, device='cuda', generator=g)
    g_enc = (torch.randn(16, M, 2, device='cuda', generator=g) * 0.1).half()
    ray_err = torch.rand(4096, device='cuda', generator=g)
    sb = slabs_b.clone()
    sb[3, 100] = float('inf')
    host = ctypes.cast(capi.host_offsets(toffs), ctypes.c_void_p)
    for with_ws in (True, False):
        gw_a, gw_b = torch.full((n_a,), float('nan'), **half), torch.full((n_b,), float('nan'), **half)
        g_emb = torch.zeros(int(offs[-1]), 2, **half)
        found, loss = torch.zeros(1, device='cuda'), torch.full((1,), float('nan'), device='cuda')
        _, ws, nbytes = capi.grid_backward_workspace(toffs, M, 3, 2, 16, S, 16, 0, 0, capi.NGP_F16) if with_ws else (None, None, 0)
        sets = capi.SlabSets(P(slabs_a), s_a, n_a, P(gw_a), P(sb), s_b, n_b, P(gw_b), P(ray_err), ray_err.numel(), P(loss))
        capi.check(lib.ngp_grid_encode_backward_checked_slabs(P(g_enc), P(x), None, P(toffs), P(g_emb), M, 3, 2, 16, S, 16, None, None, 0, 0, 0, capi.NGP_F16,
                                                              1.0, host, P(ws), nbytes, P(found), ctypes.cast(ctypes.pointer(sets), ctypes.c_void_p), st))
        out = dict(grad_weights_a=gw_a, grad_weights_b=gw_b, found_inf=found, loss=loss)
        if with_ws:
            out['grad_embeddings'] = g_emb   # the record-sort path: deterministic (without a workspace the table is scattered with atomics)
        keep(f'grid/workspace={with_ws}', 0, **out)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **saved)
    finite = sum(int(np.isfinite(a.astype(np.float64)).sum()) for a in saved.values() if a.dtype != np.uint8)
    print(f'{capi.LIB_PATH}: {len(saved)} arrays, {sum(a.nbytes for a in saved.values())} bytes, {finite} finite values -> {out_path}')


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    bad = n_bytes = 0
    for key in sorted(a.files):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        n_bytes += x.nbytes
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8))
        if not same:
            bad += 1
            where = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))[:4] if x.shape == y.shape and x.dtype == y.dtype else None
            print(f'DIFFERENT {key}: {x.dtype}{x.shape} against {y.dtype}{y.shape}, first differing bytes {where}')
    print(f'{len(a.files)} arrays ({n_bytes} bytes) compared, {bad} differ')
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
