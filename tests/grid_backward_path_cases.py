"""Tables, inputs and the call of tests/test_gpu_grid_backward_paths.py, shared with tools/grid_backward_bits.py (which stores every array
these calls write, for a comparison of two builds).  The inputs are numpy + oracle only; `run` needs a GPU.

Three small tables, all fp16 with two features, at the smallest batches that take the record-sort path (B = 16384 = BIN_MIN_SAMPLES = 32
chunks of 512 samples, and B = 16421: a partly filled last chunk).  What the plan rule (plan_backward, csrc/gridencoder.hip) makes of them
is asserted on the CPU by tests/test_grid_backward_abi.py::test_plan_rule_of_the_three_small_tables:
  T1  D = 3, 8 levels, 8 -> x 1.9, 2^15: three dense round-robin levels (736, 4920, 27000 entries), five hashed levels of 8 slices; every
      level sorted, the 128-counter sort kernel
  T2  the same with D = 2: five dense and three hashed levels
  T3  D = 3, 4 levels, 64 -> x 1.5, 2^20 (3 284 464 entries): level 0 dense round-robin; level 1 dense with 912 680 entries, too large for
      round-robin bins: an ATOMIC level riding in the sort's launch; levels 2-3 hashed with 256 slices: the 512-counter sort kernel
Fully sorted calls are exact integer sums whatever the inputs (ray-ordered samples, fp16-rounded gradients with a block of exact zeros).  A
call with an atomic level takes samples on the half lattice of THAT level (grid_lattice_cases.level_lattice): its sums have no rounding, so
the undefined order of the fp16 atomics cannot show, and every equality the tests state holds bit for bit by construction."""
import ctypes
import functools

import numpy as np

import grid_lattice_cases as glc
import oracle

SMALL = dict(num_levels=8, level_dim=2, per_level_scale=1.9, base_resolution=8, log2_hashmap_size=15)
TABLES = dict(T1=dict(input_dim=3, **SMALL), T2=dict(input_dim=2, **SMALL),
              T3=dict(input_dim=3, num_levels=4, level_dim=2, per_level_scale=1.5, base_resolution=64, log2_hashmap_size=20))
ATOMIC_LEVEL = dict(T3=1)
BATCHES = (16384, 16421)
SLICE = 4096             # BIN_SLICE
DENSE_BINS = 128         # BIN_DENSE_BINS


@functools.lru_cache(maxsize=None)
def table(name, align=False):
    cfg = TABLES[name]
    offs, pls = oracle.grid_offsets(align_corners=align, **cfg)
    offs.setflags(write=False)
    return dict(name=name, offs=offs, S=float(np.log2(pls)), H=cfg['base_resolution'], D=cfg['input_dim'], L=cfg['num_levels'])


def level_scale(tab, level):
    return float(oracle.grid_level_table(tab['L'], tab['S'], tab['H'])[0][level])


@functools.lru_cache(maxsize=None)
def ray_inputs(name, B, seed=0, magnitude=0.1):
    """x [B, D], g [L, B, 2] float32 holding fp16 values: ray-ordered samples (runs on the coarse levels), the edge points of the unit cube, a
    block of exactly-zero gradients"""
    tab = table(name)
    rng = np.random.default_rng(900 + seed)
    x = glc.ray_points(-(-B // 64), 64, tab['D'], rng)[:B].copy()
    x[0], x[1], x[2] = 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))
    x[3, 0] = -1e-7
    g = oracle.round_fp16(rng.normal(size=(tab['L'], B, 2)).astype(np.float32) * magnitude)
    g[:, 1000:1100] = 0.0
    for a in (x, g):
        a.setflags(write=False)
    return x, g


@functools.lru_cache(maxsize=None)
def lattice_inputs(name, B, level, seed=0):
    """x, g as above, but the samples sit on the half lattice of `level` and that level's gradient is J * 2^-6: the sums AT THAT LEVEL are exact
    in fp16 in any order (checked here with the oracle against the table's own offsets)"""
    tab = table(name)
    x, J = glc.level_lattice(B, tab['D'], level_scale(tab, level), seed)
    rng = np.random.default_rng(950 + seed)
    g = oracle.round_fp16(rng.normal(size=(tab['L'], B, 2)).astype(np.float32) * 0.1)
    g[:, 1000:1100] = 0.0
    g[level] = J * 2.0 ** -6
    glc.level_lattice_exact(x, g[level], tab['offs'], level, tab['S'], tab['H'])
    g.setflags(write=False)
    return x, g


def inputs(name, B, seed=0):
    return lattice_inputs(name, B, ATOMIC_LEVEL[name], seed) if name in ATOMIC_LEVEL else ray_inputs(name, B, seed)


def resized(offs, level, size):
    """the offsets of the same table with one level of another size"""
    sizes = np.diff(offs).astype(np.int64)
    sizes[level] = size
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def run(tab, x, g, entry='ws', gridtype=0, align=False, interp=0, offs=None, host_offs=None, ge=None, found_inf=False, sets=None, ws_fill=0xAB):
    """one backward call through `entry` ('ws' | 'checked' | 'slabs').  offs: the device offsets (default: the table's), host_offs: the host copy
    the plan is made from (default: the device offsets); ge: the table the call adds into (default: zeros); sets: a _ngp_capi.SlabSets, passed
    to 'slabs' only.  -> dict(ge, found_inf (tensor or None), ws (the raw workspace after the call), nbytes)"""
    import torch
    import _ngp_capi as capi
    offs = tab['offs'] if offs is None else offs
    host_offs = offs if host_offs is None else host_offs
    L, B, C = g.shape
    D = x.shape[1]
    gt, xt, ot = torch.from_numpy(np.array(g)).cuda().half(), torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(offs)).cuda()
    if ge is None:
        ge = torch.zeros(int(offs[-1]), C, device='cuda', dtype=torch.half)
    arr = (ctypes.c_int32 * len(host_offs))(*[int(v) for v in host_offs])
    hp = ctypes.cast(arr, ctypes.c_void_p)
    S, H = tab['S'], tab['H']
    nbytes = int(capi.lib.ngp_grid_backward_workspace_bytes(hp, B, D, C, L, S, H, gridtype, int(align), capi.NGP_F16))
    assert nbytes > 0, 'this call must take the record-sort path'
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device='cuda')
    fi = torch.zeros(1, device='cuda') if found_inf else None
    head = (gt.data_ptr(), xt.data_ptr(), None, ot.data_ptr(), ge.data_ptr(), B, D, C, L, S, H, None, None, gridtype, int(align), interp, capi.NGP_F16, 0.0,
            hp, ws.data_ptr(), nbytes)
    if entry == 'ws':
        assert fi is None and sets is None
        rc = capi.lib.ngp_grid_encode_backward_ws(*head, capi.stream())
    elif entry == 'checked':
        assert sets is None
        rc = capi.lib.ngp_grid_encode_backward_checked(*head, capi.ptr(fi), capi.stream())
    else:
        rc = capi.lib.ngp_grid_encode_backward_checked_slabs(*head, capi.ptr(fi), None if sets is None else ctypes.byref(sets), capi.stream())
    capi.check(rc)
    torch.cuda.synchronize()
    return dict(ge=ge, found_inf=fi, ws=ws, nbytes=nbytes)


def record_keys(ws, n_bins, B, D):
    """the 16-bit keys of all records a call left in its workspace, per binned level (n_bins: bins of each binned level, in order).  Layout
    (BinPlan and k_grid_backward_bin, csrc/gridencoder.hip): descriptors [level][bin][chunk] = first pair unit | records << 16, padded to 256
    bytes; then per (level, chunk) an area of 512 * 2^D record slots of 8 bytes holding pair units of three words {key 0 | key 1 << 16, value 0,
    value 1}.  Key bits 0x8000 / 0x4000: channel 0 / 1 of the value is 1/64 of the contribution."""
    raw = ws.cpu().numpy()
    chunks = -(-B // 512)
    total_desc = sum(n_bins) * chunks
    desc = raw[:4 * total_desc].view(np.uint32)
    words = raw[(4 * total_desc + 255) // 256 * 256:]
    words = words[:len(words) // 4 * 4].view(np.uint32)
    area = 512 * (1 << D) * 2
    out, base = [], 0
    for li, nb in enumerate(n_bins):
        keys = []
        d = desc[base:base + nb * chunks].reshape(nb, chunks)
        for b, c in zip(*np.nonzero(d >> 16)):
            first, cnt = int(d[b, c] & 0xffff), int(d[b, c] >> 16)
            w = words[(li * chunks + c) * area + 3 * first + 3 * np.arange((cnt + 1) // 2)]
            keys.append(np.stack([w & 0xffff, w >> 16], 1).reshape(-1)[:cnt])
        out.append(np.concatenate(keys) if keys else np.zeros(0, np.uint32))
        base += nb * chunks
    return out
