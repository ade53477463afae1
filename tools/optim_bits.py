"""Every output bit of the optimizer's C entries (csrc/optim.hip) and of the grid backward's fused table sweep (csrc/gridencoder.hip with
`table_adam`), for a same-box comparison of two builds of libngp_hip.so.

    NGP_HIP_LIBRARY=<one build> python tools/optim_bits.py --out a.npz        (a fresh process per library)
    NGP_HIP_LIBRARY=<other build> python tools/optim_bits.py --out b.npz
    python tools/optim_bits.py --compare a.npz b.npz                            (no GPU; exit status 1 on any difference)

Covered: ngp_optim_adam_step_ex over the phase subsets optim.py issues (CHECK|UPDATE|COMMIT, UPDATE|COMMIT, CHECK, UPDATE, COMMIT alone) x
fp16 / fp32 gradients x keep bit x clean / overflowing steps, with and without the folded EMA, on a wide-path tensor, an odd-length
misaligned one and a short one; a nine-tensor chunked NGPAdam.step(); ngp_optim_adam_small_commit with and without a table prefix, flip on
and off, clean and skipped; ngp_optim_ema_update; ngp_optim_poison_shards / ngp_optim_shard_verdict; ngp_grid_table_adam_prefix and
ngp_grid_encode_backward_checked_slabs with table_adam on a two-level table (one dense, one hashed level) at 16384 samples, followed by the
closing launch.  Every buffer an entry writes is stored whole together with the eight state words; buffers an entry must fill are NaN-filled
first, the table gradient (which the overwriting backward fills) too.  The comparison is on the bytes."""
import argparse
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

RULE = (0.9, 0.99, 1e-15, 1.0, 2.0, 0.5, 2.0)   # beta1, beta2, eps, grad_mult, growth, backoff, growth_interval (2: the scale grows in a run)
CHECK, UPDATE, COMMIT = 1, 2, 4
SIZES = (4104, 4103, 37)                         # the wide path; pair loop + odd tail (views one element into their allocations); a short tensor


def run(out_path):
    import torch
    import _ngp_capi as capi
    import fused
    from gridencoder import GridEncoder
    from optim import FOUND_INF, TABLE_PARITY, NGPAdam, announce_overwrite
    lib, vp = capi.lib, ctypes.c_void_p
    saved = {}
    gen = torch.Generator().manual_seed(7)

    def keep(case, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            assert f'{case}/{name}' not in saved
            saved[f'{case}/{name}'] = t.detach().cpu().numpy()

    def state(found_inf=0.0, scale=128.0, parity=0.0):
        return torch.tensor([scale, 1.0, found_inf, 3.0, 0.5, parity, 0.0, 0.0], device='cuda')

    def place(t, offset):
        """on the device; offset: one element into a larger allocation"""
        if not offset:
            return t.cuda()
        big = torch.zeros(t.numel() + 8, dtype=t.dtype, device='cuda')
        big[1:1 + t.numel()].copy_(t)
        return big[1:1 + t.numel()]

    def tensors(half, overflow, ema):
        out = []
        for n in SIZES:
            g = torch.randn(n, generator=gen) * 4.0
            g[::7] = 0.0
            g[3::11] = 2.0 ** -22
            g[5::13] = 65504.0
            if overflow and n == SIZES[1]:
                g[n // 2] = float('inf')
            off = n == SIZES[1]
            p = torch.randn(n, generator=gen) * 1e-2
            out.append(dict(n=n, p=place(p, off), m=place(torch.randn(n, generator=gen) * 1e-3, off), v=place(torch.rand(n, generator=gen) * 1e-6, off),
                            g=place(g.half() if half else g.half().float(), off), p16=place(p.half(), off) if half else None,
                            ema=place(p + 1e-3, off) if ema else None))
        return out

    def arrays(ts, is_half, ema):
        k = len(ts)
        col = lambda name: (vp * k)(*[None if t[name] is None else t[name].data_ptr() for t in ts])
        raw = [(ctypes.c_uint64 * k)(*[t['n'] for t in ts]), col('p'), col('m'), col('v'), col('g'), col('p16'), (ctypes.c_int * k)(*[is_half] * k),
               (ctypes.c_float * k)(*[1e-2, 3e-3, 1e-3][:k]), col('ema') if ema else None]
        return raw, [None if a is None else ctypes.cast(a, vp) for a in raw]

    def dump(case, ts, st):
        for i, t in enumerate(ts):
            keep(f'{case}/tensor{i}', **{k: v for k, v in t.items() if k != 'n' and v is not None})
        keep(case, state=st)

    # ---- ngp_optim_adam_step_ex ----
    for phases, half, kept, overflow, ema in itertools.product((CHECK | UPDATE | COMMIT, UPDATE | COMMIT, CHECK, UPDATE), (True, False), (False, True),
                                                               (False, True), (False, True)):
        if (kept and not half) or (ema and not phases & UPDATE):
            continue
        ts = tensors(half, overflow, ema)
        st = state(1.0 if overflow and not phases & CHECK else 0.0)   # (without the sweep the producers have raised the flag)
        raw, cast = arrays(ts, (1 if half else 0) | (2 if kept else 0), ema)
        capi.check(lib.ngp_optim_adam_step_ex(len(ts), *cast[:8], *RULE, st.data_ptr(), cast[8], 0.01 if ema else 0.0, phases, capi.stream()))
        dump(f'step_ex/phases={phases},half={half},keep={kept},overflow={overflow},ema={ema}', ts, st)
    for found_inf, scale in ((0.0, 128.0), (1.0, 128.0), (0.0, 1e-45), (0.0, 2.0 ** 127)):
        st = state(found_inf, scale)
        capi.check(lib.ngp_optim_adam_step_ex(0, *[None] * 8, *RULE, st.data_ptr(), None, 0.0, COMMIT, capi.stream()))
        keep(f'step_ex/commit_only/found_inf={found_inf},scale={scale}', state=st)

    # ---- a nine-tensor step: two chunks, CHECK x 2 -> UPDATE x 2 -> COMMIT ----
    for overflow in (False, True):
        torch.manual_seed(11)
        params = [torch.nn.Parameter(torch.randn(64 + 8 * i, device='cuda') * 0.1) for i in range(9)]
        opt = NGPAdam(params, lr=1e-2, init_scale=128.0, growth_interval=2)
        for step in range(3):
            for i, p in enumerate(params):
                p._ngp_grad16.copy_((torch.randn(p.numel(), generator=gen) * 2.0).half())
            if overflow and step == 1:
                params[8]._ngp_grad16[5] = float('nan')
            opt.step()
        for i, p in enumerate(params):
            keep(f'nine_tensors/overflow={overflow}/tensor{i}', p=p.data, m=opt.state[p]['exp_avg'], v=opt.state[p]['exp_avg_sq'], p16=p._ngp_fp16, g=p._ngp_grad16)
        keep(f'nine_tensors/overflow={overflow}', state=opt.scalars)

    # ---- ngp_optim_adam_small_commit ----
    for prefix, flip, found_inf, parity in itertools.product((0, 4104), (0, 1), (0.0, 1.0), (0.0, 1.0)):
        if parity and not prefix:
            continue
        ts = tensors(True, False, False)[1:]
        st = state(found_inf, parity=parity)
        raw, cast = arrays(ts, 1, False)
        sets, ta, tg = None, None, None
        if prefix:
            sets = [dict(p=torch.randn(prefix, generator=gen).cuda() * 1e-2, m=torch.randn(prefix, generator=gen).cuda() * 1e-3,
                         v=torch.rand(prefix, generator=gen).cuda() * 1e-6) for _ in range(2)]
            for s in sets:
                s['p16'] = s['p'].half()
            for k in ('p', 'm', 'v', 'p16'):
                sets[1 - int(parity)][k].fill_(float('nan'))      # the set a standing step writes whole
            tg = (torch.randn(prefix, generator=gen) * 4.0).half().cuda()
            ta = capi.TableAdam()
            for field, k in (('param', 'p'), ('exp_avg', 'm'), ('exp_avg_sq', 'v'), ('param_fp16', 'p16')):
                getattr(ta, field)[0], getattr(ta, field)[1] = sets[0][k].data_ptr(), sets[1][k].data_ptr()
            ta.state = st.data_ptr()
            ta.lr, ta.beta1, ta.beta2, ta.eps = 2e-2, 0.9, 0.99, 1e-15
        capi.check(lib.ngp_optim_adam_small_commit(len(ts), *cast[:8], *RULE, st.data_ptr(), flip, None if ta is None else ctypes.cast(ctypes.pointer(ta), vp),
                                                   capi.ptr(tg), prefix, capi.stream()))
        case = f'small_commit/prefix={prefix},flip={flip},found_inf={found_inf},parity={parity}'
        dump(case, ts, st)
        for i, s in enumerate(sets or []):
            keep(f'{case}/set{i}', **s)
        if prefix:
            keep(case, table_grad=tg)

    # ---- ngp_optim_ema_update ----
    ts = tensors(False, False, True)
    raw, cast = arrays(ts, 0, True)
    capi.check(lib.ngp_optim_ema_update(len(ts), cast[0], cast[1], cast[8], 0.05, capi.stream()))
    for i, t in enumerate(ts):
        keep(f'ema_update/tensor{i}', ema=t['ema'], p=t['p'])

    # ---- the shard kernels ----
    shards, payload = 4, 1000
    for found_inf in (0.0, 1.0):
        flat = (torch.randn(shards * payload, generator=gen)).half().cuda()
        st = state(found_inf)
        capi.check(lib.ngp_optim_poison_shards(flat.data_ptr(), shards, payload, st.data_ptr(), capi.stream()))
        keep(f'poison_shards/found_inf={found_inf}', flat=flat, state=st)
        st2 = state(0.0)
        capi.check(lib.ngp_optim_shard_verdict(flat[payload:].data_ptr(), st2.data_ptr(), flat.data_ptr(), shards, payload, capi.stream()))
        keep(f'shard_verdict/found_inf={found_inf}', flat=flat, state=st2)

    # ---- the table's Adam sweep inside the grid backward + the closing launch: two levels (17^3 dense, 2^14 hashed), 16384 samples ----
    M, L, H = 16384, 2, 16
    for overflow in (False, True):
        torch.manual_seed(3)
        enc = GridEncoder(input_dim=3, num_levels=L, level_dim=2, base_resolution=H, log2_hashmap_size=14, desired_resolution=64).cuda()
        with torch.no_grad():
            enc.embeddings.uniform_(-0.5, 0.5)
        small = torch.nn.Parameter(torch.randn(7168, device='cuda') * 0.1)
        opt = NGPAdam([{'params': [enc.embeddings], 'lr': 1e-2}, {'params': [small], 'lr': 3e-3}], betas=(0.9, 0.99), eps=1e-15, init_scale=128.0,
                      growth_interval=2)
        opt.enable_table_fusion(enc.embeddings)
        emb, S = enc.embeddings, float(np.log2(enc.per_level_scale))
        arr = capi.host_offsets(enc.offsets)
        prefix = int(lib.ngp_grid_table_adam_prefix(ctypes.cast(arr, vp), M, 3, 2, L, S, H, enc.gridtype_id, 0, capi.NGP_F16))
        assert prefix == int(enc.offsets[1]), (prefix, enc.offsets)
        for step in range(3):
            x = torch.rand(M, 3, generator=gen).cuda()
            g_enc = (torch.randn(L, M, 2, generator=gen) * 0.05).half().cuda()
            if overflow and step == 1:
                g_enc[1, 123, 1] = float('inf')
            small._ngp_grad16.copy_((torch.randn(7168, generator=gen) * 0.01).half())
            emb._ngp_grad16.fill_(float('nan'))    # the overwriting backward stores the dense levels' gradient; the rest is left to it as well
            fused._grid_backward(g_enc, x, enc.offsets, emb._ngp_grad16, M, L, S, H, enc.gridtype_id, 0, enc.interp_id, 0.0, capi.stream(),
                                 found_inf=opt.scalars.narrow(0, FOUND_INF, 1), slabs=None, overwrite=True, table_adam=opt.table_adam())
            announce_overwrite(emb, table_adam_prefix=prefix)
            case = f'table_adam/overflow={overflow}/step{step}'
            st, alt = opt.state[emb], opt._table_alt
            keep(case + '/backward', state=opt.scalars, grad_prefix=emb._ngp_grad16[:prefix], p0=emb.data, m0=st['exp_avg'], v0=st['exp_avg_sq'], h0=st['fp16'],
                 p1=alt['p'], m1=alt['m'], v1=alt['v'], h1=alt['p16'])
            opt.step(gradients_checked=True)
            keep(case + '/step', state=opt.scalars, p0=emb.data, m0=st['exp_avg'], v0=st['exp_avg_sq'], h0=st['fp16'], p1=alt['p'], m1=alt['m'],
                 v1=alt['v'], h1=alt['p16'], small=small.data, small_m=opt.state[small]['exp_avg'], small_v=opt.state[small]['exp_avg_sq'],
                 small_h=small._ngp_fp16, small_g=small._ngp_grad16)
        assert prefix > 0 and float(opt.scalars[TABLE_PARITY]) in (0.0, 1.0)

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
