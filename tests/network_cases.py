"""Cases, references and criteria shared by tests/test_network_cases.py (CPU) and tests/test_gpu_network_kernels.py (GPU): the fused network
kernels behind the grid encoder -- ngp_network_forward / _rows, ngp_network_backward_color, ngp_ffmlp_backward_ex in the planar layouts,
ngp_ffmlp_reduce_slabs_pair -- and the glue kernels of csrc/pipeline.hip, against a float64 model of network_ff.py:51-74 with the fp16
rounding points of pipeline.hip:1-9 and include/ngp_hip.h ("The whole network ... in ONE launch").  numpy only.

STAGES (each at dtype=np.float64: the DEFINITION; at np.float32: every operation and accumulation rounded to fp32, exp evaluated in fp32 --
the yardstick of the fp32 kernels' rounding, the role composite_model(np.float32) has in render_loop_cases):
    sigma_stage     enc (row-major [M,32] or planar [16][M][2], element [l][m][c] = feature 2l+c) -> h16       oracle.ffmlp_forward
    mid_forward     sigma = density_scale * exp(h0), color_in = [half(SH_4(dir)) | h16[:,1:16] | 0]; rows >= M_valid use dir = 0
    color_stage     color_in -> out16                                                                           oracle.ffmlp_forward
    rgb_forward     half(sigmoid(out16[:, :3]))
    rgb_backward    half(g * (y * (1 - y))) in columns 0..2, zeros in 3..15
    color_backward  -> dL/dcolor_in [M,32], g_wc                                                                oracle.ffmlp_backward
    mid_backward    column 0 = half((density_scale * g_sigma) * exp(clip(h0, -15, 15))) (np.clip: a NaN stays a NaN), 1..15 = g_color_in[:,16:31]
    sigma_backward  -> planar g_enc [16][M][2], g_ws                                                            oracle.ffmlp_backward
The MLPs run with round_hidden=True.  SH_4 is `sh4`, the polynomials of csrc/sh_poly.inc in numpy (oracle.sh_forward is an fp32 C kernel and
could not serve as a float64 definition; test_network_cases pins sh4 to it); trunc_exp is written out at `dtype` and pinned to
oracle.trunc_exp_forward / _backward the same way.  Every glue stage also returns its value BEFORE the last rounding (`*_pre`).

CRITERIA (coded once here, applied by the CPU test to the float32 twin and to the wrong variants and by the
GPU test to the kernels).  Every model stage is evaluated from the STORED upstream tensors of the implementation under test (h16, color_in,
g_h16: "teacher forcing"), so one fp16 ulp upstream does not widen the next bar:
    MLP outputs               rtol 1e-3, atol 1e-3 * max|ref| (test_gpu_ffmlp.py), the maximum taken per column block (h0 | features)
    dL/dx through ReLU masks  close_except_relu_flips(tol=4e-3, bulk=0.995)
    weight gradients          max / L2 error relative to the gradient's scale under 3e-3 / 2e-3 x max(1, nl - 1)
    glue from exact inputs    `yardstick`: 4 x max|float32 model - float64 definition| + 1e-7 x max|reference|, applied to the value before
                              the output's rounding; the output must lie between the roundings of (definition -/+ bound) -- an fp16 output
                              one fp32 rounding away from a tie may land on either neighbour, never further.  Products (sigma, column 0 of
                              g_h16, g_out16) span tens of binades, so their yardstick is the same rule on the RELATIVE error (plus 4 fp32
                              subnormal steps); NaN / +inf / -inf are compared by class.
    copies                    exact by value (-0 == 0)

WRONG_VARIANTS are deliberately wrong models; the CPU test shows that each fails a criterion on the cases below.
CASES: `nominal`, `wide_h0` (row 0 of the sigma net's output matrix times 2**WIDE[nl_s][1]: h0 beyond +-15 on both sides), `glue_table`
(hand-written rows), `mse_cases`, `pad_cases`."""
import functools
import math

import numpy as np

import oracle

WRONG_VARIANTS = ('clamp at 16', 'no clamp', 'NaN h0 -> exp(-15)', 'density_scale dropped in the backward', 'features h[:,0:15]',
                  'pad column non-zero', 'SH halves swapped', 'planar input read as row-major', 'planar dL/dx written row-major',
                  'rgb not rounded to fp16', 'tail rows use the last valid direction')

DS_FORWARD, DS_BACKWARD = 1.7, 1.3
F32_TINY = 4.0 * 2.0 ** -149


def n_params(nl):
    return 64 * (32 + 64 * (nl - 1) + 16)


def layers_of(w):
    nl = (np.asarray(w).size // 64 - 48) // 64 + 1
    assert n_params(nl) == np.asarray(w).size
    return nl


def half(a, dtype=np.float64):
    """round to the nearest fp16 (overflow -> inf), as a `dtype` array"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(a).astype(np.float16).astype(dtype)


def to_rows(enc):
    """planar [16][M][2] -> row-major [M,32] (feature 2l+c); a 2-d array is taken as row-major already"""
    enc = np.asarray(enc)
    return enc if enc.ndim == 2 else enc.transpose(1, 0, 2).reshape(enc.shape[1], 32)


def to_planar(x):
    x = np.asarray(x)
    return np.ascontiguousarray(x.reshape(x.shape[0], 16, 2).transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------
# the stages
# ------------------------------------------------------------------------------------------------
def sh4(d, dtype=np.float64):
    """the 16 real SH components of degree < 4 in the expression order of csrc/sh_poly.inc (shencoder.cu:60-98), at `dtype`"""
    f = dtype
    d = np.asarray(d, dtype=f).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = f
    xx, yy, zz = x * x, y * y, z * z
    out = [np.full_like(x, c(0.28209479177387814)),
           c(-0.48860251190291992) * y, c(0.48860251190291992) * z, c(-0.48860251190291992) * x,
           c(1.0925484305920791) * x * y, c(-1.0925484305920791) * y * z, c(0.94617469575756002) * zz - c(0.31539156525252001),
           c(-1.0925484305920791) * x * z, c(0.54627421529603954) * xx - c(0.54627421529603954) * yy,
           y * (c(-1.7701307697799305) * xx + c(0.59004358992664351) * yy), c(2.8906114426405541) * x * y * z,
           c(-2.2852289973223287) * y * zz + c(0.45704579946446574) * y, z * (c(1.865881662950577) * zz - c(1.1195289977703462)),
           c(-2.2852289973223287) * x * zz + c(0.45704579946446574) * x, z * (c(1.445305721320277) * xx - c(1.445305721320277) * yy),
           c(-0.59004358992664351) * (x * x * x) + c(1.7701307697799305) * x * yy]
    out = np.stack(out, 1)
    assert out.dtype == f
    return out


def sigma_stage(enc, w_sigma, nl_s=None, dtype=np.float64, variant=None):
    """-> h16 [M,16] (fp16 values at `dtype`)"""
    nl_s = nl_s or layers_of(w_sigma)
    enc = np.asarray(enc)
    x = enc.reshape(enc.shape[1], 32) if (variant == 'planar input read as row-major' and enc.ndim == 3) else to_rows(enc)
    out, _ = oracle.ffmlp_forward(x, w_sigma, 32, 16, 64, nl_s, round_hidden=True, dtype=dtype)
    return half(out, dtype)


def mid_forward(h16, dirs, M_valid, density_scale, dtype=np.float64, variant=None):
    """-> dict: sigma [M] (at `dtype`, before the fp32 store), sh_pre [M,16] (before the fp16 rounding), color_in [M,32]"""
    f = dtype
    h = np.asarray(h16, dtype=f)
    M = h.shape[0]
    d = np.zeros((M, 3), f)
    d[:M_valid] = np.asarray(dirs, dtype=f)[:M_valid]
    if variant == 'tail rows use the last valid direction' and 0 < M_valid < M:
        d[M_valid:] = d[M_valid - 1]
    with np.errstate(over='ignore', invalid='ignore'):
        sigma = f(np.float32(density_scale)) * np.exp(h[:, 0])        # (density_scale crosses the ABI as a float)
    sh = sh4(d, f)
    if variant == 'SH halves swapped':
        sh = np.concatenate([sh[:, 8:], sh[:, :8]], 1)
    feat = h[:, 0:15] if variant == 'features h[:,0:15]' else h[:, 1:16]
    pad = h[:, 15:16] + f(1.0) if variant == 'pad column non-zero' else np.zeros((M, 1), f)
    return dict(sigma=sigma, sh_pre=sh, color_in=np.concatenate([half(sh, f), feat, pad], 1))


def color_stage(color_in, w_color, nl_c=None, dtype=np.float64):
    """-> out16 [M,16]"""
    nl_c = nl_c or layers_of(w_color)
    out, _ = oracle.ffmlp_forward(np.asarray(color_in), w_color, 32, 16, 64, nl_c, round_hidden=True, dtype=dtype)
    return half(out, dtype)


def sigmoid(v):
    with np.errstate(over='ignore', invalid='ignore'):
        one = v.dtype.type(1.0)
        return one / (one + np.exp(-v))


def rgb_forward(out16, dtype=np.float64, variant=None, pre=False):
    s = sigmoid(np.asarray(out16, dtype=dtype)[:, :3])
    return s if (pre or variant == 'rgb not rounded to fp16') else half(s, dtype)


def rgb_backward(g_rgb, rgb, dtype=np.float64, pre=False):
    """-> g_out16 [M,16] (pre: columns 0..2 before the rounding, [M,3])"""
    f = dtype
    g, y = np.asarray(g_rgb, dtype=f), np.asarray(rgb, dtype=f)
    with np.errstate(over='ignore', invalid='ignore'):
        p = g * (y * (f(1.0) - y))
    return p if pre else np.concatenate([half(p, f), np.zeros((g.shape[0], 13), f)], 1)


def color_backward(g_out16, color_in, w_color, dtype=np.float64):
    """-> (dL/dcolor_in [M,32], g_wc)"""
    nl = layers_of(w_color)
    _, fb = oracle.ffmlp_forward(np.asarray(color_in), w_color, 32, 16, 64, nl, round_hidden=True, dtype=dtype)
    return oracle.ffmlp_backward(g_out16, color_in, w_color, fb, 32, 16, 64, nl, round_hidden=True, dtype=dtype)


def mid_backward(g_sigma, h16, g_color_in, density_scale, dtype=np.float64, variant=None, pre=False):
    """-> g_h16 [M,16] (pre: column 0 before the rounding, [M])"""
    f = dtype
    h0 = np.asarray(h16, dtype=f)[:, 0]
    ds = f(1.0) if variant == 'density_scale dropped in the backward' else f(np.float32(density_scale))
    with np.errstate(over='ignore', invalid='ignore'):
        if variant == 'clamp at 16':
            e = np.exp(np.clip(h0, f(-16.0), f(16.0)))
        elif variant == 'no clamp':
            e = np.exp(h0)
        else:
            e = np.exp(np.clip(h0, f(-15.0), f(15.0)))
        if variant == 'NaN h0 -> exp(-15)':
            e = np.where(np.isnan(h0), np.exp(f(-15.0)), e)
        p = (ds * np.asarray(g_sigma, dtype=f)) * e
    if pre:
        return p
    return np.concatenate([half(p, f)[:, None], np.asarray(g_color_in, dtype=f)[:, 16:31]], 1)


def sigma_backward(g_h16, enc, w_sigma, dtype=np.float64, variant=None):
    """-> (planar g_enc [16][M][2], g_ws)"""
    nl = layers_of(w_sigma)
    enc = np.asarray(enc)
    x = enc.reshape(enc.shape[1], 32) if (variant == 'planar input read as row-major' and enc.ndim == 3) else to_rows(enc)
    _, fb = oracle.ffmlp_forward(x, w_sigma, 32, 16, 64, nl, round_hidden=True, dtype=dtype)
    gx, gw = oracle.ffmlp_backward(g_h16, x, w_sigma, fb, 32, 16, 64, nl, round_hidden=True, dtype=dtype)
    if variant == 'planar dL/dx written row-major':
        return np.ascontiguousarray(gx).reshape(16, gx.shape[0], 2), gw
    return to_planar(gx), gw


# ------------------------------------------------------------------------------------------------
# an implementation of the whole chain on a case (the float32 twin, a wrong variant): what the GPU launches produce
# ------------------------------------------------------------------------------------------------
def shift_column0(g_h16, shift):
    """column 0 times 2**-shift, re-rounded to fp16 (exact unless it lands in the subnormals): what both sides feed the sigma net's backward
    in the wide_h0 case (see `wide_h0`)"""
    g = np.array(g_h16, copy=True)
    if shift:
        g[:, 0] = half(g[:, 0] * 2.0 ** -shift, g.dtype)
    return g


def _f32(a):
    """what an fp32 store keeps of a value (overflow -> inf)"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(a).astype(np.float32)


def run_forward(case, dtype, variant=None, planar=True):
    enc = case['enc_planar'] if planar else case['enc']
    h16 = sigma_stage(enc, case['w_sigma'], case['nl_s'], dtype, variant)
    mid = mid_forward(h16, case['dirs'], case['M_valid'], DS_FORWARD, dtype, variant)
    rgb = rgb_forward(color_stage(mid['color_in'], case['w_color'], case['nl_c'], dtype), dtype, variant)
    return dict(h16=h16, sigma=_f32(mid['sigma']), color_in=mid['color_in'], rgb=rgb)


def run_backward(case, fwd, dtype, variant=None):
    """the backward launches on the forward's stored h16 / color_in -> g_h16, g_wc, g_enc (planar), g_ws"""
    g_cin, g_wc = color_backward(case['g_out16'], fwd['color_in'], case['w_color'], dtype)
    g_h16 = mid_backward(case['g_sigma'], fwd['h16'], half(g_cin, dtype), DS_BACKWARD, dtype, variant)
    g_enc, g_ws = sigma_backward(shift_column0(g_h16, case['shift']), case['enc_planar'], case['w_sigma'], dtype, variant)
    return dict(g_h16=g_h16, g_wc=g_wc, g_enc=half(g_enc, dtype), g_ws=g_ws)


# ------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------
def relu_flip_figures(got, ref, tol):
    """the three figures of test_gpu_ffmlp's dL/dx comparison -> (share of entries within tol, share of rows within 2 tol, median row error)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.abs(got - ref) <= tol * np.abs(ref) + tol * np.abs(ref).max()
    row_err = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1).mean()
    return float(ok.mean()), float((row_err < 2 * tol).mean()), float(np.median(row_err))


def close_except_relu_flips(got, ref, tol, bulk=0.995):
    """dL/dx goes through ReLU masks taken from fp16 activations: a pre-activation within rounding distance of 0 may be
    masked on one side and not on the other, which changes single entries by a whole weight column.  Require the bulk to
    agree element-wise and the tensor to agree in norm."""
    share, rows, median = relu_flip_figures(got, ref, tol)
    assert share > bulk, share
    assert rows > 0.99 and median < tol


def _model_error(pre64, pre32, relative):
    """max error of the float32 model over the entries whose definition is finite (relative: and non-zero and fp32-normal)"""
    a, b = np.asarray(pre64, np.float64), np.asarray(pre32, np.float64)
    keep = np.isfinite(a) & np.isfinite(b)
    if relative:
        keep &= (np.abs(a) > 2.0 ** -100) & (np.abs(a) < 2.0 ** 100)
    if not keep.any():
        return 0.0, 0.0
    err = np.abs(b[keep] - a[keep]) / (np.abs(a[keep]) if relative else 1.0)
    return float(err.max()), (1.0 if relative else float(np.abs(a[keep]).max()))


RELATIVE = {'sigma': True, 'sh': False, 'rgb': False, 'g_out16': True, 'g_h0': True, 'loss': False}


def yardstick(name, src):
    """4 x (max error of the float32 model against the float64 definition on the same inputs) + 1e-7 x (largest reference magnitude) -- the
    rule of composite_geo_cases.yardstick -- for glue output `name` on the inputs in `src` (a case merged with its reference's h16, or the
    glue table), taken before the output's own rounding; relative error for the products (RELATIVE).  -> (bound, float32 model error)"""
    pair = []
    for f in (np.float64, np.float32):
        if name == 'sigma':
            pair.append(mid_forward(src['h16'], src['dirs'], src['M_valid'], src.get('ds_forward', DS_FORWARD), f)['sigma'])
        elif name == 'sh':
            pair.append(mid_forward(src['h16'], src['dirs'], src['M_valid'], DS_FORWARD, f)['sh_pre'])
        elif name == 'rgb':
            pair.append(rgb_forward(src['out16'], f, pre=True))
        elif name == 'g_out16':
            pair.append(rgb_backward(src['g_rgb'], src['rgb'], f, pre=True))
        elif name == 'g_h0':
            pair.append(mid_backward(src['g_sigma'], src['h16'], None, DS_BACKWARD, f, pre=True))
        elif name == 'loss':
            pair.append(mse_model(src['image'], src['target'], src['scale'], f)[0])
        else:
            raise KeyError(name)
    err, scale = _model_error(pair[0], pair[1], RELATIVE[name])
    return 4.0 * err + 1e-7 * scale, err


def within(got, pre, bound, relative, fmt):
    """per entry: the output `got` lies between the roundings (to the output format `fmt`, np.float16 or np.float32) of pre -/+ bound;
    a NaN definition wants a NaN; +-inf wants the same infinity.  -> (ok [bool array], n_off: entries that are not the nearest rounding of
    `pre`, worst: over those entries, the distance of `pre` from the rounding tie between `got` and the nearest rounding in units of the bound
    -- at most 1 for an output next to the nearest one; 0 if every entry is the nearest rounding)"""
    got, pre = np.asarray(got, np.float64), np.asarray(pre, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        b = np.where(np.isfinite(pre), bound * np.abs(pre) + F32_TINY if relative else bound, 0.0)
        lo, hi = (pre - b).astype(fmt).astype(np.float64), (pre + b).astype(fmt).astype(np.float64)
        nearest = pre.astype(fmt).astype(np.float64)
    nan = np.isnan(pre)
    with np.errstate(invalid='ignore'):
        ok = np.where(nan, np.isnan(got), (got >= lo) & (got <= hi))
        off = ~nan & ~(got == nearest)
        sel = off & np.isfinite(pre) & np.isfinite(got) & np.isfinite(nearest) & (b > 0)
        worst = float((np.abs(pre - 0.5 * (got + nearest))[sel] / b[sel]).max()) if sel.any() else 0.0
    return ok, int(off.sum()), worst


class Report(list):
    """rows (name, ok, figure, bar, note)"""
    def add(self, name, ok, figure, bar, note=''):
        self.append((name, bool(ok), figure, bar, note))

    def failures(self):
        return [r for r in self if not r[1]]

    def __str__(self):
        return '\n'.join(f'{"ok  " if ok else "FAIL"} {name:28s} {fig!s:>24s}  bar {bar!s:<22s} {note}' for name, ok, fig, bar, note in self)


def _mlp_bar(rep, name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    excess = np.abs(got - ref) - (1e-3 * np.abs(ref) + 1e-3 * scale)
    fin = np.isfinite(got).all()
    rep.add(name, fin and float(excess.max()) <= 0.0, float(np.abs(got - ref).max() / scale) if fin else np.nan, '1e-3 (+1e-3 rel)',
            f'{int((got != ref).sum())} of {got.size} entries differ')


def _exact(rep, name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    rep.add(name, not bad.any(), int(bad.sum()), 'exact')


def forward_criteria(got, case):
    """`got`: h16 [M,16], sigma [M], color_in [M,32], rgb [M,3] of one implementation of the forward -> Report"""
    rep = Report()
    ref = reference(case)
    h16, cin, rgb = (np.asarray(got[k], np.float64) for k in ('h16', 'color_in', 'rgb'))
    _mlp_bar(rep, 'h16[:,0]', h16[:, :1], ref['h16'][:, :1])
    _mlp_bar(rep, 'h16[:,1:16]', h16[:, 1:], ref['h16'][:, 1:])
    mid = mid_forward(h16, case['dirs'], case['M_valid'], DS_FORWARD)
    b, _ = case_yardstick('sigma', case)
    ok, off, worst = within(got['sigma'], mid['sigma'], b, True, np.float32)
    rep.add('sigma', ok.all(), worst, f'{b:.2e} rel', f'{off} entries off the nearest fp32')
    b, _ = case_yardstick('sh', case)
    ok, off, worst = within(cin[:, :16], mid['sh_pre'], b, False, np.float16)
    rep.add('SH block', ok.all(), worst, f'{b:.2e} abs', f'{off} entries off the nearest fp16')
    _exact(rep, 'SH(0) behind M_valid', cin[case['M_valid']:, :16], np.broadcast_to(half(sh4(np.zeros((1, 3)), np.float32)), (len(cin) - case['M_valid'], 16)))
    _exact(rep, 'feature shuffle', cin[:, 16:31], h16[:, 1:16])
    _exact(rep, 'zero pad', cin[:, 31], np.zeros(len(cin)))
    out = color_stage(cin, case['w_color'], case['nl_c'])
    bar = 1e-3 * np.abs(out[:, :3]) + 1e-3 * float(np.abs(out).max())
    y, _ = yardstick('rgb', dict(out16=out))
    lo, hi = half(sigmoid(out[:, :3] - bar) - y), half(sigmoid(out[:, :3] + bar) + y)
    ok = (rgb >= lo) & (rgb <= hi)
    want = half(sigmoid(out[:, :3]))
    rep.add('rgb', ok.all(), float(np.abs(rgb - want).max()), f'{float((hi - lo).max() / 2):.2e} abs (out16 bar through the sigmoid)',
            f'{int((rgb != want).sum())} of {rgb.size} entries differ')
    _exact(rep, 'rgb == half(rgb)', rgb, half(rgb))
    return rep


def _wgrad(rep, name, got, ref, nl):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    flips = max(1, nl - 1)
    fin = bool(np.isfinite(got).all())
    e_max = float(np.abs(got - ref).max() / np.abs(ref).max()) if fin else np.nan
    e_l2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref)) if fin else np.nan
    rep.add(name + ' max', fin and e_max < 3e-3 * flips, e_max, 3e-3 * flips)
    rep.add(name + ' L2', fin and e_l2 < 2e-3 * flips, e_l2, 2e-3 * flips)


def _dx(rep, name, got, ref):
    fin = bool(np.isfinite(np.asarray(got, np.float64)).all())
    share, rows, median = relu_flip_figures(got, ref, 4e-3) if fin else (np.nan,) * 3
    rep.add(name, fin and share > 0.995 and rows > 0.99 and median < 4e-3, (round(share, 5), round(rows, 5), float(f'{median:.2e}')) if fin else np.nan,
            '(>0.995, >0.99, <4e-3)')


def backward_criteria(got, fwd, case):
    """`got`: g_h16 [M,16], g_wc, g_enc [16][M][2], g_ws of one implementation of the backward launches on the forward's stored `fwd`
    (h16, color_in) -> Report"""
    rep = Report()
    g_h16 = np.asarray(got['g_h16'], np.float64)
    pre = mid_backward(case['g_sigma'], fwd['h16'], None, DS_BACKWARD, pre=True)
    b, _ = case_yardstick('g_h0', case)
    ok, off, worst = within(g_h16[:, 0], pre, b, True, np.float16)
    rep.add('g_h16[:,0]', ok.all(), worst, f'{b:.2e} rel', f'{off} entries off the nearest fp16')
    g_cin, g_wc = color_backward(case['g_out16'], fwd['color_in'], case['w_color'])
    _dx(rep, 'g_h16[:,1:16]', g_h16[:, 1:], g_cin[:, 16:31])
    _wgrad(rep, 'g_wc', got['g_wc'], g_wc, case['nl_c'])
    g_enc, g_ws = sigma_backward(shift_column0(g_h16, case['shift']), case['enc_planar'], case['w_sigma'])
    _dx(rep, 'g_enc (planar)', to_rows(got['g_enc']), to_rows(g_enc))
    _wgrad(rep, 'g_ws', got['g_ws'], g_ws, case['nl_s'])
    return rep


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _rng(seed, item):
    return np.random.default_rng([seed, item])


def _r16(a):
    return oracle.round_fp16(a)


def _build(nl_s, nl_c, M, seed, power):
    assert M % 128 == 0 and M >= 128
    scale = math.sqrt(3 / 64)
    w_sigma = _r16(_rng(seed, 0).uniform(-1, 1, n_params(nl_s)) * scale)
    if power:
        w_sigma[-16 * 64:-15 * 64] *= 2.0 ** power            # row 0 of the output matrix [16,64]: still exact in fp16
        assert np.array_equal(w_sigma, _r16(w_sigma))
    w_color = _r16(_rng(seed, 1).uniform(-1, 1, n_params(nl_c)) * scale)
    enc = _r16(_rng(seed, 2).uniform(-0.5, 0.5, (M, 32)))      # (row m is the same for every M: the draws are sequential)
    M_valid = M - 37
    d = _rng(seed, 3).normal(size=(M_valid, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[5:69] *= _rng(seed, 4).uniform(0.3, 2.5, (64, 1))                                     # 64 non-normalised
    d[70:78] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1]], np.float64)   # 8 axis-aligned
    d[78:82] = 0.0                                                                          # 4 zero directions
    g_out16 = _r16(_rng(seed, 5).normal(size=(M, 16)) * 0.05)
    g_out16[g_out16 == 0] = 2.0 ** -10
    g_sigma = (_rng(seed, 6).normal(size=M) * 1e-3).astype(np.float32)
    return dict(nl_s=nl_s, nl_c=nl_c, M=M, M_valid=M_valid, w_sigma=w_sigma, w_color=w_color, enc=enc, enc_planar=to_planar(enc),
                dirs=d.astype(np.float32), g_out16=g_out16, g_sigma=g_sigma, shift=0, seed=seed, power=power)


@functools.lru_cache(maxsize=4)
def nominal(nl_s, nl_c, M):
    """enc ~ U(-0.5, 0.5), weights U(-1, 1) * (3/64)**0.5, all pre-rounded to fp16; unit directions, 64 non-normalised, 8 axis-aligned and 4
    zero ones, M_valid = M - 37 direction rows; g_out16 ~ N(0, 0.05) with all 16 columns non-zero, g_sigma ~ N(0, 1e-3).  density_scale is
    DS_FORWARD = 1.7 in the forward and DS_BACKWARD = 1.3 in the backward.  Treat as read-only."""
    return _build(nl_s, nl_c, M, 1000 + 10 * nl_s + nl_c, 0)


# nl_s -> (seed, power of two on row 0 of the sigma net's output matrix, shift): searched once on the CPU for the conditions of `wide_h0` at
# every M of WIDE_M, then frozen (test_network_cases re-checks them)
WIDE = {2: (2, 7, 12), 3: (5, 8, 12), 4: (2, 9, 12)}
WIDE_M = (128, 256, 384, 512, 1024, 4224, 33408, 131200)


@functools.lru_cache(maxsize=4)
def wide_h0(nl_s, nl_c, M):
    """`nominal` with another seed and row 0 of the sigma net's output matrix times a power of two (WIDE), so that in the float64 definition
    at least 2 % of the rows have h0 < -15, at least 2 % h0 > 15, every h0 < 80 (finite sigma) and |column 0 of g_h16| < 65504.
    The clamped rows carry |g_h16[:,0]| of a few thousand; times the scaled weight row that overflows the fp16 hidden gradients of the sigma
    net's backward (inf * 0 on the masked units: nothing to compare).  The sigma net's backward of this case is therefore fed g_h16 with
    column 0 times 2**-shift (`shift_column0`, an exact scaling) on both sides; column 0 itself is checked on the unscaled values."""
    seed, power, shift = WIDE[nl_s]
    return dict(_build(nl_s, nl_c, M, 5000 + seed, power), shift=shift)


CASES = {'nominal': nominal, 'wide_h0': wide_h0}


@functools.lru_cache(maxsize=4)
def _reference(kind, nl_s, nl_c, M):
    case = CASES[kind](nl_s, nl_c, M)
    return dict(h16=sigma_stage(case['enc'], case['w_sigma'], nl_s))


def reference(case):
    """the float64 definition's h16 of a case (computed once)"""
    return _reference('wide_h0' if case['power'] else 'nominal', case['nl_s'], case['nl_c'], case['M'])


@functools.lru_cache(maxsize=64)
def _case_yardstick(name, kind, nl_s, nl_c, M):
    case = CASES[kind](nl_s, nl_c, M)
    return yardstick(name, dict(case, h16=_reference(kind, nl_s, nl_c, M)['h16']))


def case_yardstick(name, case):
    """`yardstick` of a case's glue output on the float64 definition's own h16 (computed once per case)"""
    return _case_yardstick(name, 'wide_h0' if case['power'] else 'nominal', case['nl_s'], case['nl_c'], case['M'])


def wide_conditions(case, backward=True):
    """-> dict of the figures `wide_h0` promises, from the float64 definition"""
    h16 = reference(case)['h16']
    h0 = h16[:, 0]
    g0 = mid_backward(case['g_sigma'], h16, None, DS_BACKWARD, pre=True)
    out = dict(below=float((h0 < -15).mean()), above=float((h0 > 15).mean()), h0_max=float(h0.max()), h0_min=float(h0.min()),
               g0_max=float(np.abs(g0).max()))
    if not backward:
        return out
    fwd = run_forward(case, np.float64)
    g_h16 = run_backward(case, fwd, np.float64)['g_h16']
    x, nl = case['enc'], case['nl_s']
    fb = oracle.ffmlp_forward(x, case['w_sigma'], 32, 16, 64, nl, dtype=np.float64)[1]
    _, _, hidden = oracle.ffmlp_backward(shift_column0(g_h16, case['shift']), x, case['w_sigma'], fb, 32, 16, 64, nl, round_hidden=False, return_hidden=True)
    return dict(out, hidden_max=float(max(np.abs(h).max() for h in hidden)))


# ------------------------------------------------------------------------------------------------
# the glue table
# ------------------------------------------------------------------------------------------------
H0_VALUES = (-np.inf, -65504.0, -16.0, -15.0078125, -15.0, -14.9921875, -0.0, 0.0, 14.9921875, 15.0, 15.0078125, 16.0, 88.0, 89.0, 65504.0, np.inf,
             np.nan)
G_SIGMA_VALUES = (0.0, 1e-45, -3e-39, 1e-3, -0.7, 1.0)       # zero, two fp32 denormals, ordinary, and 1.0: 1.3 * exp(15) overflows fp16
OUT_VALUES = (65504.0, -65504.0, np.inf, -np.inf, 17.0, -17.0, 8.0, -8.0, 0.0, np.nan, 2.0 ** -24, 0.5, -1.25)
G_RGB_VALUES = (0.0, 1e-42, 1e-3, -2.5, 3e5, -3e5)           # 3e5 * y (1 - y) overflows fp16 around y = 0.5


@functools.lru_cache(maxsize=None)
def glue_table():
    """hand-written rows for the four glue kernels: every h0 of H0_VALUES with every g_sigma of G_SIGMA_VALUES (102 rows), out16[:, :3]
    cycling through OUT_VALUES and g_rgb through G_RGB_VALUES so that every pair meets; columns 1..15 of h16 hold row + column / 16 and
    g_color_in holds -(row % 50 + column / 32) (all exact in fp16): a shifted or swapped column is an exact mismatch.  rgb is the
    definition's rgb_forward(out16).  -> dict (M = M_valid = 102, dirs: unit vectors)"""
    T = len(H0_VALUES) * len(G_SIGMA_VALUES)
    r = np.arange(T)
    h16 = r[:, None] + np.arange(16)[None, :] / 16.0
    h16[:, 0] = np.array(H0_VALUES)[r % len(H0_VALUES)]
    g_sigma = np.array(G_SIGMA_VALUES, np.float32)[r // len(H0_VALUES)]
    g_color_in = -((r % 50)[:, None] + np.arange(32)[None, :] / 32.0)
    out16 = (r[:, None] * 0.25 + np.arange(16)[None, :]) % 7.0 - 3.0
    for c in range(3):
        out16[:, c] = np.array(OUT_VALUES)[(r + 5 * c) % len(OUT_VALUES)]
    g_rgb = np.stack([np.array(G_RGB_VALUES, np.float32)[(r // len(OUT_VALUES) + c) % len(G_RGB_VALUES)] for c in range(3)], 1)
    d = np.random.default_rng(9).normal(size=(T, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.array_equal(half(h16), h16, equal_nan=True) and np.array_equal(half(g_color_in), g_color_in) and np.array_equal(half(out16), out16, equal_nan=True)
    return dict(M=T, M_valid=T, h16=h16, g_sigma=g_sigma, g_color_in=g_color_in, out16=out16, g_rgb=g_rgb, rgb=rgb_forward(out16).astype(np.float32),
                dirs=d.astype(np.float32), ds_forward=DS_FORWARD)


def run_glue(table, dtype, variant=None):
    """the four glue kernels on the table, as an implementation at `dtype`"""
    mid = mid_forward(table['h16'], table['dirs'], table['M_valid'], DS_FORWARD, dtype, variant)
    return dict(sigma=_f32(mid['sigma']), color_in=mid['color_in'], rgb=rgb_forward(table['out16'], dtype, variant),
                g_out16=rgb_backward(table['g_rgb'], table['rgb'], dtype),
                g_h16=mid_backward(table['g_sigma'], table['h16'], table['g_color_in'], DS_BACKWARD, dtype, variant))


def _tiled(a, rows):
    a = np.asarray(a)
    return a[np.arange(rows) % len(a)]


def tiled_table(rows):
    """the table repeated to `rows` rows"""
    t = glue_table()
    out = {k: (_tiled(v, rows) if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    out.update(M=rows, M_valid=rows)
    return out


def glue_criteria(got, table, only=None):
    """`got`: sigma, color_in, rgb, g_out16, g_h16 (any subset named by `only`) of the glue kernels on `table` -> Report; finite expectations
    by yardstick (of the untiled table), NaN / +inf / -inf by class, copies exact"""
    rep = Report()
    base = glue_table()
    keys = only or ('sigma', 'color_in', 'rgb', 'g_out16', 'g_h16')
    mid = mid_forward(table['h16'], table['dirs'], table['M_valid'], DS_FORWARD)
    if 'sigma' in keys:
        b, _ = yardstick('sigma', base)
        ok, off, worst = within(got['sigma'], mid['sigma'], b, True, np.float32)
        rep.add('table sigma', ok.all(), worst, f'{b:.2e} rel', f'{off} off nearest; failing rows {np.flatnonzero(~ok)[:8].tolist()}')
    if 'color_in' in keys:
        cin = np.asarray(got['color_in'], np.float64)
        b, _ = yardstick('sh', base)
        ok, off, worst = within(cin[:, :16], mid['sh_pre'], b, False, np.float16)
        rep.add('table SH block', ok.all(), worst, f'{b:.2e} abs', f'{off} off nearest')
        _exact(rep, 'table feature shuffle', cin[:, 16:31], table['h16'][:, 1:16])
        _exact(rep, 'table zero pad', cin[:, 31], np.zeros(len(cin)))
    if 'rgb' in keys:
        b, _ = yardstick('rgb', base)
        ok, off, worst = within(got['rgb'], rgb_forward(table['out16'], pre=True), b, False, np.float16)
        rep.add('table rgb', ok.all(), worst, f'{b:.2e} abs', f'{off} off nearest; failing rows {np.flatnonzero(~ok.all(1))[:8].tolist()}')
        _exact(rep, 'table rgb == half(rgb)', got['rgb'], half(got['rgb']))
    if 'g_out16' in keys:
        g = np.asarray(got['g_out16'], np.float64)
        b, _ = yardstick('g_out16', base)
        ok, off, worst = within(g[:, :3], rgb_backward(table['g_rgb'], table['rgb'], pre=True), b, True, np.float16)
        rep.add('table g_out16[:, :3]', ok.all(), worst, f'{b:.2e} rel', f'{off} off nearest; failing rows {np.flatnonzero(~ok.all(1))[:8].tolist()}')
        _exact(rep, 'table g_out16[:, 3:]', g[:, 3:], np.zeros((len(g), 13)))
    if 'g_h16' in keys:
        g = np.asarray(got['g_h16'], np.float64)
        b, _ = yardstick('g_h0', base)
        ok, off, worst = within(g[:, 0], mid_backward(table['g_sigma'], table['h16'], None, DS_BACKWARD, pre=True), b, True, np.float16)
        rep.add('table g_h16[:,0]', ok.all(), worst, f'{b:.2e} rel', f'{off} off nearest; failing rows {np.flatnonzero(~ok)[:8].tolist()}')
        if 'g_color_in' in table and g.shape[1] == 16 and not only:
            _exact(rep, 'table g_h16[:,1:16]', g[:, 1:], table['g_color_in'][:, 16:31])
    return rep


# ------------------------------------------------------------------------------------------------
# ngp_pipeline_mse_loss and ngp_pad_2d_fp16
# ------------------------------------------------------------------------------------------------
MSE_N = (1, 63, 64, 1023, 1024, 1025, 3 * 4099)
MSE_SCALES = (None, 1024.0)


def mse_cases():
    """-> list of dicts: n, scale (None: the NULL loss_scale), image, target [n] fp32"""
    out = []
    for n in MSE_N:
        for scale in MSE_SCALES:
            rng = np.random.default_rng(300 + n)
            out.append(dict(n=n, scale=scale, image=rng.uniform(0, 1, n).astype(np.float32), target=rng.uniform(0, 1, n).astype(np.float32)))
    return out


def mse_model(image, target, scale, dtype):
    """-> (loss, grad_image).  float64: the mean of the squares and 2/n * diff * scale.  float32: the statements of k_mse_loss -- 1024 lanes
    stride through the values with acc = fma(diff, diff, acc), a shuffle tree over each wave of 64, one over the 16 partial sums, / n; the
    gradient as (fl32(2) / fl32(n) * diff) * scale"""
    n = len(image)
    s = 1.0 if scale is None else scale
    if dtype == np.float64:
        d = np.asarray(image, np.float64) - np.asarray(target, np.float64)
        return float((d * d).mean()), 2.0 / n * d * s
    f = np.float32
    d = np.asarray(image, f) - np.asarray(target, f)
    acc = np.zeros(1024, f)
    for lo in range(0, n, 1024):
        c = d[lo:lo + 1024].astype(np.float64)
        acc[:len(c)] = (c * c + acc[:len(c)].astype(np.float64)).astype(f)      # fma: the product is exact in a double, one rounding to fp32
    v = acc.reshape(16, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
    p = v[:, 0].copy()
    for off in (8, 4, 2, 1):
        p[:off] = p[:off] + p[off:2 * off]
    return float(p[0] / f(n)), (f(2.0) / f(n) * d) * f(s)


# (src_rows, src_cols, src_row_stride, dst_rows, dst_cols)
PAD_CASES = ((100, 30, 30, 128, 32),      # the row / column padding the MLP wants
             (100, 30, 37, 128, 32),      # stride > src_cols
             (0, 5, 5, 128, 16),          # nothing to copy: all zeros
             (128, 32, 32, 128, 32),      # src == dst shape: a plain copy
             (3, 5, 8, 7, 9),             # 63 destination elements: less than one block
             (257, 3, 3, 385, 17))        # 6545 destination elements: not a multiple of 256, more than one block


def pad_cases():
    """-> list of (args, src [max(src_rows, 1) * stride] fp16-valued, expected dst [dst_rows, dst_cols]); src holds distinct non-zero values,
    also in the stride gaps (which must not be copied)"""
    out = []
    for sr, sc, st, dr, dc in PAD_CASES:
        src = half(1.0 + (np.arange(max(sr, 1) * st) % 1999) / 4.0)
        want = np.zeros((dr, dc))
        if sr:
            want[:sr, :sc] = src.reshape(sr, st)[:, :sc]
        out.append(((sr, sc, st, dr, dc), src, want))
    return out
