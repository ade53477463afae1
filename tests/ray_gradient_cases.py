"""Cases and float64 models shared by tests/test_ray_gradient_abi.py (CPU) and tests/test_gpu_ray_gradient.py (GPU): the camera-pose
gradients through the training rays (csrc/ray_gradient.hip).  numpy / torch on the CPU only.

Semantics (include/ngp_hip.h): a sample of ray n is x_i = clamp(o_n + t_i d_n, -bound, bound) with the marcher's t_i as constants;
m_ij = |x_ij| < bound; a row of `rays` with count 0 or offset + count > M owns no samples.
  t_i          = sum_j m_ij d_j (x_ij - o_j) / sum_j m_ij d_j^2
  grad_o[n,j]  = sum_i m_ij g_x[i,j]
  grad_d[n,j]  = sum_i t_i m_ij g_x[i,j] + sum_i g_dir[i,j] + (J_SH4(d_n)^T sum_i g_sh[i,0:16])_j
  grad_x[i,j]  = 1 / (2 bound) sum_l sum_c g_enc[l,i,c] dy_dx[i,l,j,c]
  grad_pose[b,r,3] = sum_n grad_o[b,n,r],  grad_pose[b,r,c] = sum_n grad_d[b,n,r] dcam[n,c]
The closed forms below are these sums in float64; test_ray_gradient_abi.py checks them against torch autograd of a per-ray loop."""
import functools

import numpy as np
import torch

import oracle
import composite_geo_cases as cg
import grid_forward_cases as gfc
import grid_lattice_cases as glc

U = 2.0 ** -24   # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------------
# 1. the ray reduction
# ---------------------------------------------------------------------------------------------------------------------
RAY_BOUND = 1.0
RAY_N, RAY_M = len(cg.RAYS), cg.M
PERM2 = [3, 8, 0, 5, 9, 1, 6, 2, 4, 7]   # a second assignment of output rows
K_MAX = 64                               # upstream gradients: integers |k| <= K_MAX times 2^-6
# (row, coordinate, sign): samples planted with a coordinate exactly at +-bound, inside the 'row' (64), 'three rows' (130) and 'long' rays
PLANTED = [(64 + 5, 0, 1.0), (64 + 63, 2, -1.0), (64 + 64 + 65 + 70, 1, 1.0), (64 + 64 + 65 + 130 + 11, 0, -1.0), (64 + 64 + 65 + 130 + 299, 2, 1.0)]


def sh4(d):
    """real SH basis, bands 0..3, of directions [..., 3] in the dtype of d (torch; the polynomial forms of shencoder.cu:43-68)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    out = [torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
           1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
           0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
           0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
           1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)]
    return torch.stack(out, -1)


def sh4_jacobian(d):
    """[N,16,3] float64: d SH4_c / d d_j at the directions d [N,3]"""
    dt = torch.tensor(np.asarray(d, np.float64), requires_grad=True)
    y = sh4(dt)
    return np.stack([torch.autograd.grad(y[:, c].sum(), dt, retain_graph=True)[0].numpy() for c in range(16)], 1)


@functools.lru_cache(maxsize=None)
def ray_case(perm=0):
    """the ray table of composite_geo_cases (N = 10, M = 1600: counts 0, 1, 63, 64, 65, 130, 300, one overflowing ray) with seeded rays, samples
    and upstream gradients.  perm = 1: the same rays with another assignment of output rows (PERM2).  Rows no fitting ray owns hold NaN in
    every per-sample array.  -> dict of numpy arrays (float32 values; g_sh float16)"""
    rng = np.random.default_rng(314)
    rays = cg.ray_table(False)['rays'].copy()
    used = cg.ray_table(False)['used']
    if perm:
        rays[:, 0] = PERM2
    o = rng.uniform(-0.5, 0.5, (RAY_N, 3)).astype(np.float32)
    d = rng.standard_normal((RAY_N, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if perm:   # ray k of the table keeps its origin and direction: they move to its new output row
        o2, d2 = np.empty_like(o), np.empty_like(d)
        o2[PERM2], d2[PERM2] = o[cg.PERM], d[cg.PERM]
        o, d = o2, d2
    ts = rng.uniform(0.1, 1.5, RAY_M).astype(np.float32)
    xyzs = np.zeros((RAY_M, 3), np.float32)
    for n, off, cnt in rays:
        if cnt and off + cnt <= RAY_M:
            sl = slice(off, off + cnt)
            x = o[n].astype(np.float64) + ts[sl, None].astype(np.float64) * d[n].astype(np.float64)   # fma: one rounding
            xyzs[sl] = np.clip(x.astype(np.float32), -RAY_BOUND, RAY_BOUND)
    for row, j, sign in PLANTED:
        xyzs[row, j] = sign * RAY_BOUND
    g_x = (rng.integers(-K_MAX, K_MAX + 1, (RAY_M, 3)) * 2.0 ** -6).astype(np.float32)
    g_dir = (rng.integers(-K_MAX, K_MAX + 1, (RAY_M, 3)) * 2.0 ** -6).astype(np.float32)
    g_sh = (rng.integers(-K_MAX, K_MAX + 1, (RAY_M, 32)) * 2.0 ** -6).astype(np.float16)   # columns 16..31 belong to the geometry features
    for a in (xyzs, ts, g_x, g_dir, g_sh):
        a[used:] = np.nan
    return dict(rays=rays, rays_o=o, rays_d=d, ts=ts, xyzs=xyzs, g_x=g_x, g_dir=g_dir, g_sh=g_sh, used=used)


def owned(rays, M):
    """[(ray index n, offset, count)] of the rows that own samples"""
    return [(int(n), int(off), int(cnt)) for n, off, cnt in rays if cnt and off + cnt <= M]


def ts_model(xyzs, rays_o, rays_d, rays, bound):
    """float64 t of every owned sample (0 elsewhere), from the arrays as stored"""
    M = len(xyzs)
    ts = np.zeros(M)
    for n, off, cnt in owned(rays, M):
        x = np.asarray(xyzs[off:off + cnt], np.float64)
        o, d = np.asarray(rays_o[n], np.float64), np.asarray(rays_d[n], np.float64)
        m = np.abs(x) < bound
        num, den = (m * d * (x - o)).sum(1), (m * d * d).sum(1)
        ts[off:off + cnt] = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
    return ts


def ray_backward_model(g_x, g_dir, g_sh, xyzs, ts, rays_d, rays, bound):
    """the closed forms in float64 -> grad_o, grad_d [N,3], S_d [N,3] (the sum of the absolute terms of grad_d) and K [N] (samples per ray)"""
    N, M = len(rays_d), len(xyzs)   # (a sub-table of `rays` leaves the other rays' rows zero)
    go, gd, S, K = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N, np.int64)
    J = sh4_jacobian(rays_d) if g_sh is not None else None
    for n, off, cnt in owned(rays, M):
        sl = slice(off, off + cnt)
        x, t, g = np.asarray(xyzs[sl], np.float64), np.asarray(ts[sl], np.float64)[:, None], np.asarray(g_x[sl], np.float64)
        m = np.abs(x) < bound
        go[n] = (m * g).sum(0)
        gd[n] = (t * m * g).sum(0)
        S[n] = np.abs(t * m * g).sum(0)
        if g_dir is not None:
            gd[n] += np.asarray(g_dir[sl], np.float64).sum(0)
            S[n] += np.abs(np.asarray(g_dir[sl], np.float64)).sum(0)
        if g_sh is not None:
            h = np.asarray(g_sh[sl, :16], np.float64)
            gd[n] += h.sum(0) @ J[n]
            S[n] += np.abs(h).sum(0) @ np.abs(J[n])
        K[n] = cnt
    return go, gd, S, K


def ray_loop_autograd(g_x, g_dir, g_sh, xyzs, ts, rays_o, rays_d, rays, bound):
    """torch autograd (float64) of  sum_i g_x[i] . x_i + g_dir[i] . d + g_sh[i,:16] . SH4(d)  with x_i = o + t_i d where the stored sample is
    not clamped, ray by ray -> grad_o, grad_d [N,3]"""
    N, M = len(rays), len(xyzs)
    o = torch.tensor(np.asarray(rays_o, np.float64), requires_grad=True)
    d = torch.tensor(np.asarray(rays_d, np.float64), requires_grad=True)
    loss = torch.zeros((), dtype=torch.float64)
    for n, off, cnt in owned(rays, M):
        for i in range(off, off + cnt):
            stored = torch.tensor(np.asarray(xyzs[i], np.float64))
            x = torch.where(stored.abs() < bound, o[n] + float(ts[i]) * d[n], stored)
            loss = loss + (torch.tensor(np.asarray(g_x[i], np.float64)) * x).sum()
            if g_dir is not None:
                loss = loss + (torch.tensor(np.asarray(g_dir[i], np.float64)) * d[n]).sum()
            if g_sh is not None:
                loss = loss + (torch.tensor(np.asarray(g_sh[i, :16], np.float64)) * sh4(d[n])).sum()
    go, gd = torch.autograd.grad(loss, (o, d))
    return go.numpy(), gd.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ngp_grid_input_gradient on the lattice: no rounding at all
# ---------------------------------------------------------------------------------------------------------------------
G_KMAX, G_SHIFT = 4, 2.0 ** -4   # upstream grad_enc: integers |k| <= 4 times 2^-4
GRID_EXACT = [gfc.fcase('raygrad', c) for c in glc.SWEEP_CASES if c.dtype == 'f16'] + \
             [gfc.fcase('raygrad-mapped', glc.make_case(3, 2, 'f16', interp=1, level_sizes=(1024, glc.dense_size(3, 17, False), 8), seed=230),
                        bound=glc.BOUND)]
GRID_EXACT_BS = (1, 63, 257)


@functools.lru_cache(maxsize=None)
def grid_upstream(fc):
    """grad_enc [L,P,2] float16 on the case's pool"""
    L, P = len(fc.base.level_sizes), fc.base.B
    rng = np.random.default_rng(9000 + fc.base.seed)
    g = (rng.integers(-G_KMAX, G_KMAX + 1, (L, P, 2)) * G_SHIFT).astype(np.float16)
    g.setflags(write=False)
    return g


def contract(g, dydx, bound):
    """grad_xyzs [P,3] float64 = 1 / (2 bound) sum_l sum_c g[l,p,c] dydx[p,l,j,c] (bound = 0: factor 1), and the sum of the absolute terms"""
    g = np.asarray(g, np.float64)
    f = 1.0 / (2.0 * bound) if bound > 0.0 else 1.0
    return f * np.einsum('lpc,pljc->pj', g, dydx), f * np.einsum('lpc,pljc->pj', np.abs(g), np.abs(dydx))


@functools.lru_cache(maxsize=None)
def grid_exact_reference(fc):
    """grid_forward_cases.reference's float64 dy_dx on the pool contracted with grid_upstream -> dict(x (as the call receives it), table,
    offs, g, want [P,3], absum [P,3], unit)"""
    ref = gfc.reference(fc)
    g = grid_upstream(fc)
    want, absum = contract(g, ref['dydx'], fc.bound)
    unit = gfc.dydx_unit(fc) * G_SHIFT * (1.0 / (2.0 * fc.bound) if fc.bound > 0.0 else 1.0)
    return dict(x=gfc.inputs(fc), table=gfc.table(fc), offs=ref['offs'], g=g, want=want, absum=absum, unit=unit, inside=ref['inside'])


# ---------------------------------------------------------------------------------------------------------------------
# 5. ngp_grid_input_gradient off the lattice
# ---------------------------------------------------------------------------------------------------------------------
OFF_B, OFF_L, OFF_H, OFF_LOG2 = 1000, 8, 16, 14
OFF_MODES = [(0, 0.0), (1, 0.0), (1, 2.0)]   # (interp, bound)


@functools.lru_cache(maxsize=None)
def grid_off_lattice(interp, bound):
    """8 levels of scale 1.3819 up to 2^14 entries (two dense, six hashed), 1000 seeded points (with grid_forward_cases' edge rows), an fp16
    table and an fp16 upstream.  The float64 model takes cells and fractions from the fp32 statements of locate (gfc.frac32).
    -> dict(x, emb, offs, S, g, want [B,3], S_abs [B,3] = the sum of |g * w * (v_hi - v_lo)| over levels, channels and corner pairs)"""
    rng = np.random.default_rng(777 + interp + int(10 * bound))
    offs, pls = oracle.grid_offsets(input_dim=3, num_levels=OFF_L, level_dim=2, per_level_scale=1.3819, base_resolution=OFF_H,
                                    log2_hashmap_size=OFF_LOG2, align_corners=False)
    S = float(np.log2(pls))
    emb = oracle.round_fp16(rng.uniform(-1, 1, (int(offs[-1]), 2)).astype(np.float32))
    x = gfc.edge_points(OFF_B, 3, rng)
    if bound > 0.0:
        x = (x * np.float32(2.0 * bound) - np.float32(bound)).astype(np.float32)
    g = (rng.standard_normal((OFF_L, OFF_B, 2)) * 0.1).astype(np.float16)
    _, dydx, levels, _ = gfc.grid_reference(x, emb, offs, S, OFF_H, 0, False, interp, bound=bound, with_dydx=True)
    want, _ = contract(g, dydx, bound)
    # the sum of the absolute terms, corner pair by corner pair
    xu = gfc.unit_inputs(x, bound)
    scale, res = oracle.grid_level_table(OFF_L, S, OFF_H)
    e64, g64 = emb.astype(np.float64), g.astype(np.float64)
    S_abs = np.zeros((OFF_B, 3))
    for l in range(OFF_L):
        f, deriv = gfc.frac32(xu, scale[l], False, interp)
        gidx, _, inside = levels[l]
        for j in range(3):
            for k in range(8):
                if (k >> j) & 1:
                    continue
                w = np.full(OFF_B, scale[l], np.float32)
                for dd in range(3):
                    if dd != j:
                        w = w * (f[:, dd] if (k >> dd) & 1 else np.float32(1) - f[:, dd])
                wd = np.abs((w * deriv[:, j]).astype(np.float64))
                diff = np.abs(e64[gidx[:, k | (1 << j)]] - e64[gidx[:, k]])
                S_abs[:, j] += np.where(inside, (wd[:, None] * diff * np.abs(g64[l])).sum(1), 0.0)
    if bound > 0.0:
        S_abs /= 2.0 * bound
    dense = [(int(res[l]) + 1) ** 3 <= int(offs[l + 1] - offs[l]) for l in range(OFF_L)]
    return dict(x=x, emb=emb, offs=offs, S=S, g=g, want=want, S_abs=S_abs, inside=levels[0][2], dense=dense)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the pose backward
# ---------------------------------------------------------------------------------------------------------------------
POSE_B, POSE_H, POSE_W = 2, 5, 7
POSE_INTRINSICS = (6.5, 6.25, 3.5, 2.5)   # fx, fy, cx, cy
POSE_NS = (1, 65, 300)


@functools.lru_cache(maxsize=None)
def pose_case(N, inds_kind):
    """inds_kind: 'shared' [N], 'per_pose' [B,N], 'none' (the full 5 x 7 frame, N ignored) -> dict(poses [B,4,4], inds or None, n, grad_o
    (integer-valued), grad_d [B,n,3])"""
    rng = np.random.default_rng(50 + N + {'shared': 0, 'per_pose': 1000, 'none': 2000}[inds_kind])
    poses = np.zeros((POSE_B, 4, 4), np.float32)
    for b in range(POSE_B):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        poses[b, :3, :3] = q
        poses[b, :3, 3] = rng.uniform(-2, 2, 3)
        poses[b, 3, 3] = 1.0
    if inds_kind == 'none':
        inds, n = None, POSE_H * POSE_W
    else:
        n = N
        inds = rng.integers(0, POSE_H * POSE_W, (n,) if inds_kind == 'shared' else (POSE_B, n)).astype(np.int64)
    grad_o = rng.integers(-8, 9, (POSE_B, n, 3)).astype(np.float32)
    grad_d = rng.standard_normal((POSE_B, n, 3)).astype(np.float32)
    return dict(poses=poses, inds=inds, n=n, grad_o=grad_o, grad_d=grad_d)


def rays_from_pixels_torch(poses, intrinsics, W, inds, n):
    """torch restatement of ngp_rays_from_pixels in the dtype of poses: -> rays_o, rays_d [B,n,3] and dcam [B,n,3]"""
    B = poses.shape[0]
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics)
    pix = torch.arange(n).expand(B, n) if inds is None else torch.as_tensor(inds).expand(B, n)
    i = (pix % W).to(poses.dtype) + 0.5
    j = torch.div(pix, W, rounding_mode='floor').to(poses.dtype) + 0.5
    xs, ys = (i - cx) / fx, (j - cy) / fy
    dcam = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    dcam = dcam / dcam.norm(dim=-1, keepdim=True)
    rays_d = torch.einsum('brc,bnc->bnr', poses[:, :3, :3], dcam)
    rays_o = poses[:, None, :3, 3].expand(B, n, 3)
    return rays_o, rays_d, dcam


def pose_backward_model(case):
    """float64 autograd of the restatement -> grad_poses [B,4,4] and S [B,3,3], the sums of the absolute terms of the rotation block"""
    poses = torch.tensor(case['poses'].astype(np.float64), requires_grad=True)
    ro, rd, dcam = rays_from_pixels_torch(poses, POSE_INTRINSICS, POSE_W, case['inds'], case['n'])
    go, gd = torch.tensor(case['grad_o'].astype(np.float64)), torch.tensor(case['grad_d'].astype(np.float64))
    (g,) = torch.autograd.grad((ro * go).sum() + (rd * gd).sum(), poses)
    S = torch.einsum('bnr,bnc->brc', gd.abs(), dcam.detach().abs())
    return g.numpy(), S.numpy()
