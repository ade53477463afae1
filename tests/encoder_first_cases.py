"""Cases, references and criteria shared by tests/test_encoder_first_cases.py (CPU) and tests/test_gpu_encoder_first_order.py (GPU): the
first-order kernels of the two small encoders -- ngp_sh_encode_forward / _backward in fp32, fp16 (k_sh_forward<half_t, 1..8, *>,
k_sh_backward<half_t>) and fp64 (k_f64_sh_fwd / k_f64_sh_bwd), ngp_freq_encode_forward / _backward -- against float64 definitions of the
same operations.  numpy, `oracle` and tools/gen_sh.py only.

DEFINITIONS (float64) and YARDSTICK MODELS (the same statements with every operation rounded to float32)
    SH values, dy_dx   the 64 polynomials of tools/gen_sh.py::basis() and their symbolic derivatives (sympy.diff), numeric factors evaluated to
                       17 digits, sympy.lambdify(..., 'numpy'): plain arithmetic in the dtype of the directions it is given (np.float64: the
                       definition; np.float32: the yardstick model, its dtype asserted), on the inputs as the kernel sees them -- fp32 values,
                       fp16 values for the half path.  oracle.sh_forward is a C kernel that stores fp32 and could not serve as a float64
                       definition (as in network_cases); test_encoder_first_cases uses it as a stand-in kernel instead.
    SH backward        want[b,d] = prior[b,d] + sum_i grad[b,i] * dy_dx[b,d,i] (include/ngp_hip.h: the entry ACCUMULATES) from the STORED
                       dy_dx of the implementation under test ("teacher forcing"); the model is the same sum in float32, sequential in i
    frequency          oracle.freq_forward / oracle.freq_backward are the float64 definition (the cosine is sin(fl32(fl32(x 2^f) + fl32(pi/2)))
                       evaluated in float64; the backward reads the STORED outputs and OVERWRITES grad_inputs); the backward's model is
                       r = g[d]; r += 2^f * (g_s * o_c - g_c * o_s) in float32

CRITERIA (coded once here, applied by the CPU test to the float32 twin, to stand-in kernels and to the wrong variants, and by the GPU test to
the kernels)
    fp32 SH values / dy_dx   per component (column): |got - def| <= 4 x max_b |float32 model - def| + 1e-7 x max_b |def| -- the rule of
                             composite_geo_cases.yardstick and network_cases.yardstick, per column because a degree-8 component is ~400
                             times band 0.  max_b runs over `yard_dirs`, the rows of all the dtype's cases together (1000 distinct
                             directions, the first 50 also unscaled): the float32 error of a column is a property of its expression on this
                             distribution of directions, and a case of one row -- (0, 0, 1), where every power of z is exact and the factored
                             model has no error at all while an expanded form with rounded coefficients has -- is no sample of it
                             (test_encoder_first_cases: an honest fp32 Horner evaluation would miss that one-row bound by 1.13).  An
                             identically zero derivative column has bound 0: exact zeros.
    fp16 SH                  the same per-column bound (of the fp16-valued directions) on the value before the output's rounding: the fp16
                             output lies between the roundings of (def -/+ bound) (network_cases.within)
    fp64 SH                  rel 1e-12 (+ 1e-14 x max(1, max|want|)), the rule of test_gpu_fp64._close, against the definition
    SH backward              fp32: `whole_yardstick` = 4 x max|float32 model - def| + 1e-7 x max|def| over the tensor; fp16: within() of that
                             bound; fp64: the rule above
    frequency forward        identity block exact by value; sines |got - oracle.freq_forward| <= 3e-7 (the project's own figure, test_freqencoder.py:
                             "accurate sinf vs float64 sine")
    frequency backward       `whole_yardstick`; deg = 0 is a copy: exact
    guard rows               every output has GUARD = 64 rows behind row B filled with a NaN bit pattern (SENTINEL); they keep their bits
An output row that was not written still holds the sentinel NaN and fails its comparison.

WRONG_VARIANTS are deliberately wrong models; the CPU test shows that each fails a criterion on the cases below.
CASES: SH degrees 1..8 x dtype (f32, f16, f64) x SH_BATCHES; directions: unit vectors, the first min(B, 100) // 2 rows scaled off the sphere by
0.2 .. 1.5, the rows (0,0,1), (1,0,0), (0,-1,0), (0,0,0) first where B allows.  Frequency: FREQ_SHAPES x FREQ_BATCHES, x ~ U(-1, 1), and the
two TRIP cases that send the grid-stride loops (at most 65536 workgroups of 256 lanes) on a second trip."""
import functools

import numpy as np

import oracle
from encoder_second_cases import gen_sh
from network_cases import Report, within

WRONG_VARIANTS_SH = ('backward overwrites', 'dy_dx laid out [B,N,3]', 'band 3 in reversed m order', 'last band left zero',
                     'last partial wave not written', 'fp16 truncated toward zero')
WRONG_VARIANTS_FREQ = ('exact cosine', 'sin / cos interleaved per dimension', 'backward without 2^f', 'backward adds into grad_inputs',
                       'elements behind 65536 * 256 dropped')
WRONG_VARIANTS = WRONG_VARIANTS_SH + WRONG_VARIANTS_FREQ

SH_DEGREES = tuple(range(1, 9))
SH_BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)     # one lane; a wave -1, =, +1; a workgroup -1, =, +1; a ragged tail of several workgroups
YARD_ROWS = 1000
FREQ_SHAPES = ((3, 4), (3, 10), (2, 6), (1, 1), (3, 0), (64, 1))   # (D, deg)
FREQ_BATCHES = (1, 64, 65, 257, 1000)
GRID_CAP = 65536 * 256                                # elements of one trip through either frequency kernel's grid-stride loop
TRIP_FORWARD = (3, 10, 266306)                        # B * C = 16 777 278 = GRID_CAP + 62: the first 62 lanes of workgroup 0 go round twice
TRIP_BACKWARD = (64, 1, 262145)                       # B * D = 16 777 280 = GRID_CAP + 64

GUARD = 64
KINDS = {'f32': np.float32, 'f16': np.float16, 'f64': np.float64}
_BITS = {'f32': (np.uint32, 0x7fc0dead), 'f16': (np.uint16, 0x7ead), 'f64': (np.uint64, 0x7ff8dead0000beef)}   # quiet NaNs with a payload


# ------------------------------------------------------------------------------------------------
# guarded buffers
# ------------------------------------------------------------------------------------------------
def guarded(rows, cols, kind):
    """[rows + GUARD, cols] in the storage dtype of `kind`, every element the sentinel"""
    u, bits = _BITS[kind]
    return np.full((rows + GUARD, cols), bits, u).view(KINDS[kind])


def sentinel_count(buf, kind):
    """number of elements of `buf` that hold the sentinel's bits"""
    u, bits = _BITS[kind]
    return int((np.ascontiguousarray(buf).view(u) == bits).sum())


def _guard(rep, name, buf, rows, kind):
    tail = np.ascontiguousarray(buf[rows:])
    rep.add(name + ' guard rows', len(buf) == rows + GUARD and sentinel_count(tail, kind) == tail.size, tail.size - sentinel_count(tail, kind), 'intact')


# ------------------------------------------------------------------------------------------------
# SH: definition and model
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sh_callables():
    """-> (Y, dY): 64 callables of (x, y, z) and 3 x 64 for d/dx, d/dy, d/dz; a constant polynomial returns a Python number"""
    import sympy as sp
    g = gen_sh()
    v = (g.x, g.y, g.z)
    lam = lambda e: sp.lambdify(v, sp.sympify(e).evalf(17), 'numpy')
    Y = g.basis()
    return tuple(lam(e) for e in Y), tuple(tuple(lam(sp.diff(e, s)) for e in Y) for s in v)


@functools.lru_cache(maxsize=None)
def sh_zero_columns():
    """-> bool [3, 64]: the derivative is identically zero"""
    import sympy as sp
    g = gen_sh()
    return np.array([[sp.diff(e, s) == 0 for e in g.basis()] for s in (g.x, g.y, g.z)])


def _columns(fns, x, y, z, dtype):
    cols = []
    for f in fns:
        c = f(x, y, z)
        cols.append(c if isinstance(c, np.ndarray) else np.full_like(x, dtype(c)))
    out = np.stack(cols, -1)
    assert out.dtype == dtype, out.dtype
    return out


def sh_eval(dirs, degree, dtype, variant=None):
    """-> (Y [B,N], dY [B,3,N]) at `dtype` on the values of `dirs`"""
    d = np.asarray(dirs).astype(dtype).reshape(-1, 3)
    x, y, z = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
    N = degree * degree
    fy, fd = sh_callables()
    with np.errstate(all='ignore'):
        Y = _columns(fy[:N], x, y, z, dtype)
        dY = np.stack([_columns(fd[s][:N], x, y, z, dtype) for s in range(3)], 1)
    if variant == 'band 3 in reversed m order' and degree >= 4:
        Y[:, 9:16] = Y[:, 9:16][:, ::-1].copy()
        dY[:, :, 9:16] = dY[:, :, 9:16][:, :, ::-1].copy()
    if variant == 'last band left zero':
        Y[:, (degree - 1) ** 2:] = 0
        dY[:, :, (degree - 1) ** 2:] = 0
    return Y, dY


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def sh_dirs(B, kind):
    """[B,3] in the storage dtype of `kind`: the first B rows of the YARD_ROWS-row set of that dtype (rows drawn one after the other; the
    scaled block and the four hand-written rows are laid over the first rows of each B).  Treat as read-only."""
    assert 1 <= B <= YARD_ROWS
    d = _unit(np.random.default_rng(77), YARD_ROWS)[:B]
    k = min(B, 100) // 2
    d[:k] *= np.random.default_rng(78).uniform(0.2, 1.5, (50, 1))[:k]
    special = np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0], [0, 0, 0]], np.float64)
    d[:min(B, 4)] = special[:min(B, 4)]
    return d.astype(np.float32).astype(KINDS[kind])


@functools.lru_cache(maxsize=None)
def yard_dirs(kind):
    """the rows the per-column yardstick is taken over: every row that occurs in a case of `kind` (the B = 1000 case and, since the scaled
    block covers fewer rows at small B, the unscaled versions of its rows)"""
    return np.concatenate([sh_dirs(B, kind) for B in SH_BATCHES])


def _model_dtype(kind):
    return np.float64 if kind == 'f64' else np.float32


@functools.lru_cache(maxsize=None)
def sh_yardstick(kind, degree=8):
    """-> dict: bound_Y [N], bound_dY [3,N] (4 x float32-model error + 1e-7 x largest definition, per column over yard_dirs(kind)), err_Y,
    err_dY (the float32 model's errors), max_Y, max_dY.  Columns of a lower degree are a prefix."""
    if degree != 8:
        full = sh_yardstick(kind, 8)
        N = degree * degree
        return {k: v[..., :N] for k, v in full.items()}
    d = yard_dirs(kind)
    Y, dY = sh_eval(d, 8, np.float64)
    Y32, dY32 = sh_eval(d, 8, np.float32)
    err_Y, err_dY = np.abs(Y32 - Y).max(0), np.abs(dY32 - dY).max(0)
    max_Y, max_dY = np.abs(Y).max(0), np.abs(dY).max(0)
    return dict(bound_Y=4.0 * err_Y + 1e-7 * max_Y, bound_dY=4.0 * err_dY + 1e-7 * max_dY, err_Y=err_Y, err_dY=err_dY, max_Y=max_Y, max_dY=max_dY)


@functools.lru_cache(maxsize=64)
def sh_definition(B, kind, degree):
    """-> (Y [B,N], dY [B,3,N]) float64 on the case's directions (computed once; read-only)"""
    return sh_eval(sh_dirs(B, kind), degree, np.float64)


def sh_grad(B, kind, degree):
    """upstream gradient [B,N] ~ U(-1, 1) and a prior content of grad_inputs [B,3], non-zero everywhere (0.5 <= |prior| < 2), in the storage
    dtype"""
    rng = np.random.default_rng([79, B])
    g = rng.uniform(-1, 1, (B, 64))[:, :degree * degree]
    prior = rng.uniform(0.5, 2.0, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))
    t = KINDS[kind]
    return np.ascontiguousarray(g.astype(np.float32).astype(t)), prior.astype(np.float32).astype(t)


def close64(got, want, rel=1e-12):
    """the rule of test_gpu_fp64._close -> (ok, largest error in units of its bound)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max(initial=0.0)))
    with np.errstate(invalid='ignore'):
        ratio = np.where(np.isfinite(got), np.abs(got - want) / bound, np.inf)
    worst = float(ratio.max(initial=0.0))
    return got.shape == want.shape and worst <= 1.0, worst


def _round_to(v, kind, variant=None):
    """values -> the storage dtype of `kind` (round to nearest even; the wrong variant truncates fp16 toward zero)"""
    t = KINDS[kind]
    with np.errstate(over='ignore'):
        out = np.asarray(v).astype(t)
    if variant == 'fp16 truncated toward zero' and kind == 'f16':
        beyond = np.abs(out.astype(np.float64)) > np.abs(np.asarray(v, np.float64))
        out = np.where(beyond, np.nextafter(out, t(0)), out)
    return out


def run_sh_forward(B, kind, degree, dtype=None, variant=None, with_grad=True):
    """the forward as an implementation that evaluates at `dtype` (default: float32 for the f32 / f16 kinds, the float32 twin; float64 for
    f64) -> dict: outputs [B+GUARD, N], dy_dx [B+GUARD, 3N] or None (guarded buffers in the storage dtype), pre_Y, pre_dY (before the
    storage rounding)"""
    dtype = dtype or _model_dtype(kind)
    N = degree * degree
    Y, dY = sh_eval(sh_dirs(B, kind), degree, dtype, variant)
    rows = (B // 64) * 64 if variant == 'last partial wave not written' else B
    out = guarded(B, N, kind)
    out[:rows] = _round_to(Y, kind, variant)[:rows]
    dy = None
    if with_grad:
        dy = guarded(B, 3 * N, kind)
        flat = dY.transpose(0, 2, 1).reshape(B, 3 * N) if variant == 'dy_dx laid out [B,N,3]' else dY.reshape(B, 3 * N)
        dy[:rows] = _round_to(flat, kind, variant)[:rows]
    return dict(outputs=out, dy_dx=dy, pre_Y=Y, pre_dY=dY)


def column_ratios(got, want, bound):
    """per column (last axis): the largest |got - want| over the rows in units of the column's bound; a column of bound 0 gives 0 if it
    is exact and inf otherwise; a NaN or inf in `got` gives inf.  `got` [B, ...cols], bound [...cols]"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(np.isfinite(got), np.abs(got - want), np.inf)
        worst = err.max(0) if len(err) else np.zeros(bound.shape)
        return np.where(worst == 0, 0.0, worst / bound)


def sh_forward_criteria(got, B, kind, degree):
    """`got`: outputs [B+GUARD, N], dy_dx [B+GUARD, 3N] or None, of one implementation on sh_dirs(B, kind) -> Report"""
    rep = Report()
    N = degree * degree
    Y, dY = sh_definition(B, kind, degree)
    out = np.asarray(got['outputs'])
    dy = None if got.get('dy_dx') is None else np.asarray(got['dy_dx'])
    assert out.dtype == KINDS[kind] and out.shape[1] == N and (dy is None or (dy.dtype == KINDS[kind] and dy.shape[1] == 3 * N))
    yd = sh_yardstick(kind, degree)
    pairs = [('values', out[:B], Y, yd['bound_Y'])]
    if dy is not None:
        pairs.append(('dy_dx', dy[:B].reshape(B, 3, N), dY, yd['bound_dY']))
    for name, g, want, bound in pairs:
        if kind == 'f32':
            r = column_ratios(g, want, bound)
            rep.add(name, r.max() <= 1.0, float(r.max()), '1 (x the column bound)', f'worst column {int(np.argmax(r))} of {r.size}; bounds {bound.min():.1e} .. {bound.max():.1e}')
            if name == 'dy_dx':
                zero = sh_zero_columns()[:, :N]
                rep.add('dy_dx zero columns', not np.any(g[:, zero] != 0), int(np.count_nonzero(g[:, zero] != 0)), 'exact zeros', f'{int(zero.sum())} columns')
        elif kind == 'f16':
            ok, off, worst = within(g, want, np.broadcast_to(bound, want.shape), False, np.float16)
            rep.add(name, ok.all(), worst, '1 (x the column bound, then fp16)', f'{off} of {ok.size} entries off the nearest fp16, {int((~ok).sum())} outside')
        else:
            ok, worst = close64(g, want)
            rep.add(name, ok, worst, '1 (x rel 1e-12)')
    _guard(rep, 'outputs', out, B, kind)
    if dy is not None:
        _guard(rep, 'dy_dx', dy, B, kind)
    return rep


# ------------------------------------------------------------------------------------------------
# SH backward
# ------------------------------------------------------------------------------------------------
def sh_backward_model(prior, grad, dy_dx, dtype, variant=None, fused=False):
    """prior [B,3], grad [B,N], dy_dx [B,3N] (values of any dtype) -> prior + sum_i grad[:,i] * dy_dx[:,d,i] at `dtype` [B,3]; float32:
    sequential in i, every product and every sum rounded (fused: each step one fma, the product exact in a double)"""
    B, N = np.asarray(grad).shape
    g = np.asarray(grad).astype(dtype)
    dd = np.asarray(dy_dx).astype(dtype).reshape(B, 3, N)
    r = np.zeros((B, 3), dtype) if variant == 'backward overwrites' else np.asarray(prior).astype(dtype).copy()
    if dtype == np.float64:
        return r + np.einsum('bi,bdi->bd', g, dd)
    for i in range(N):
        if fused:
            r = (g[:, None, i].astype(np.float64) * dd[:, :, i].astype(np.float64) + r.astype(np.float64)).astype(np.float32)
        else:
            r = r + g[:, None, i] * dd[:, :, i]
    assert r.dtype == dtype
    return r


def run_sh_backward(prior_buf, grad, dy_dx, B, kind, dtype=None, variant=None, fused=False):
    """the backward as an implementation on a guarded grad_inputs buffer holding the prior -> a new guarded buffer"""
    dtype = dtype or _model_dtype(kind)
    out = np.array(prior_buf, copy=True)
    out[:B] = _round_to(sh_backward_model(prior_buf[:B], grad, np.asarray(dy_dx)[:B], dtype, variant, fused), kind)
    return out


def whole_yardstick(model32, definition):
    """4 x max|float32 model - definition| + 1e-7 x max|definition| over the tensor -> (bound, float32 model error)"""
    a = np.asarray(definition, np.float64)
    err = float(np.abs(np.asarray(model32, np.float64) - a).max(initial=0.0))
    return 4.0 * err + 1e-7 * float(np.abs(a).max(initial=0.0)), err


def sh_backward_criteria(got_buf, prior, grad, dy_dx, B, kind):
    """`got_buf` [B+GUARD, 3]: grad_inputs after one call that found `prior` [B,3] there, with `grad` and the stored `dy_dx` -> Report"""
    rep = Report()
    got = np.asarray(got_buf)
    assert got.dtype == KINDS[kind]
    dy = np.asarray(dy_dx)[:B]
    want = sh_backward_model(prior, grad, dy, np.float64)
    g = got[:B].astype(np.float64)
    if kind == 'f64':
        ok, worst = close64(g, want)
        rep.add('grad_inputs', ok, worst, '1 (x rel 1e-12)')
    else:
        bound, err = whole_yardstick(sh_backward_model(prior, grad, dy, np.float32), want)
        if kind == 'f32':
            with np.errstate(invalid='ignore'):
                e = float(np.where(np.isfinite(g), np.abs(g - want), np.inf).max())
            rep.add('grad_inputs', e <= bound, e, f'{bound:.2e}', f'float32 model error {err:.2e}')
        else:
            ok, off, worst = within(g, want, bound, False, np.float16)
            rep.add('grad_inputs', ok.all(), worst, f'1 (x {bound:.2e}, then fp16)', f'{off} of {ok.size} entries off the nearest fp16; float32 model error {err:.2e}')
    _guard(rep, 'grad_inputs', got, B, kind)
    return rep


# ------------------------------------------------------------------------------------------------
# frequency encoder
# ------------------------------------------------------------------------------------------------
def freq_case(D, deg, B):
    """-> (x [B,D] ~ U(-1, 1), grad [B,C] ~ N(0, 1)) fp32"""
    rng = np.random.default_rng([80, D, deg, B])
    return rng.uniform(-1, 1, (B, D)).astype(np.float32), rng.standard_normal((B, D + 2 * D * deg), dtype=np.float32)


def freq_forward_model(x, deg, dtype, variant=None):
    """[B,D] fp32 -> [B,C] at `dtype`: float64 is oracle.freq_forward; float32 evaluates the same arguments with the float32 sine"""
    x = np.asarray(x, np.float32)
    B, D = x.shape
    if variant is None and dtype == np.float64:
        return oracle.freq_forward(x, deg)
    half_pi = np.float32(np.float32(3.141592653589793) / np.float32(2))
    blocks = []
    for f in range(deg):
        arg = x * np.float32(2.0 ** f)
        s = np.sin(arg.astype(dtype))
        c = np.cos(x.astype(np.float64) * 2.0 ** f).astype(dtype) if variant == 'exact cosine' else np.sin((arg + half_pi).astype(dtype))
        blocks.append((s, c))
    if variant == 'sin / cos interleaved per dimension':
        cols = [np.stack([s, c], -1).reshape(B, 2 * D) for s, c in blocks]
    else:
        cols = [np.concatenate([s, c], 1) for s, c in blocks]
    out = np.concatenate([x.astype(dtype)] + cols, 1)
    assert out.dtype == dtype
    return out


def run_freq_forward(x, deg, dtype=np.float32, variant=None):
    """-> guarded fp32 outputs [B+GUARD, C]"""
    B, D = x.shape
    C = D + 2 * D * deg
    out = guarded(B, C, 'f32')
    out[:B] = freq_forward_model(x, deg, dtype, variant).astype(np.float32)
    if variant == 'elements behind 65536 * 256 dropped' and B * C > GRID_CAP:
        out.reshape(-1)[GRID_CAP:B * C] = guarded(0, 1, 'f32')[0, 0]
    return out


CHUNK = 1 << 16          # rows per step of the frequency criteria: the trip cases have 16.7 M elements, their float64 images stay small


def freq_forward_criteria(got_buf, x, deg):
    rep = Report()
    B, D = x.shape
    got = np.asarray(got_buf)
    assert got.dtype == np.float32 and got.shape[1] == D + 2 * D * deg
    n_bad, e, first = 0, 0.0, None
    for lo in range(0, B, CHUNK):
        want = freq_forward_model(x[lo:lo + CHUNK], deg, np.float64)
        g = got[lo:min(lo + CHUNK, B)].astype(np.float64)
        n_bad += int((g[:, :D] != want[:, :D]).sum())
        with np.errstate(invalid='ignore'):
            err = np.where(np.isfinite(g[:, D:]), np.abs(g[:, D:] - want[:, D:]), np.inf)
        if first is None and err.max(initial=0.0) > 3e-7:
            r, c = np.argwhere(err > 3e-7)[0]
            first = (lo + int(r), D + int(c))
        e = max(e, float(err.max(initial=0.0)))
    rep.add('identity block', n_bad == 0, n_bad, 'exact')
    rep.add('sines', e <= 3e-7, e, 3e-7, f'first failing (row, column) {first}')
    _guard(rep, 'outputs', got, B, 'f32')
    return rep


def freq_backward_model(grad, outputs, D, deg, dtype, variant=None, contracted=False):
    """grad, stored outputs [B,C] fp32 -> [B,D] at `dtype` (float32: r = g[d]; r += 2^f * (g_s * o_c - g_c * o_s), every operation rounded;
    contracted: g_s * o_c - g_c * o_s as one fma around the rounded second product, r += 2^f * (.) as one fma -- what a compiler
    that contracts makes of the same statement)"""
    if variant is None and dtype == np.float64:
        return oracle.freq_backward(grad, outputs, D, deg)
    g, o = np.asarray(grad, np.float32).astype(dtype), np.asarray(outputs, np.float32).astype(dtype)
    r = g[:, :D].copy()
    for f in range(deg):
        s, c = slice(D + 2 * f * D, D + 2 * f * D + D), slice(D + 2 * f * D + D, D + 2 * f * D + 2 * D)
        scale = dtype(1.0) if variant == 'backward without 2^f' else dtype(2.0 ** f)
        if contracted:
            p2 = (g[:, c] * o[:, s]).astype(np.float64)
            inner = (g[:, s].astype(np.float64) * o[:, c].astype(np.float64) - p2).astype(np.float32)
            r = (np.float64(scale) * inner.astype(np.float64) + r.astype(np.float64)).astype(np.float32)
        else:
            r = r + scale * (g[:, s] * o[:, c] - g[:, c] * o[:, s])
    assert r.dtype == dtype
    return r


def run_freq_backward(grad, outputs, D, deg, dtype=np.float32, variant=None, contracted=False):
    """-> guarded fp32 grad_inputs [B+GUARD, D]; the buffer holds the sentinel before the call (the entry overwrites)"""
    B = len(grad)
    out = guarded(B, D, 'f32')
    r = freq_backward_model(grad, np.asarray(outputs)[:B], D, deg, dtype, variant, contracted).astype(np.float32)
    if variant == 'backward adds into grad_inputs':
        r = out[:B] + r
    out[:B] = r
    if variant == 'elements behind 65536 * 256 dropped' and B * D > GRID_CAP:
        out.reshape(-1)[GRID_CAP:B * D] = guarded(0, 1, 'f32')[0, 0]
    return out


def freq_backward_criteria(got_buf, grad, outputs, D, deg):
    """`got_buf` [B+GUARD, D] of one implementation on `grad` and the stored `outputs` -> Report"""
    rep = Report()
    B = len(grad)
    got = np.asarray(got_buf)
    assert got.dtype == np.float32 and got.shape[1] == D
    e, err32, scale, n_diff = 0.0, 0.0, 0.0, 0
    for lo in range(0, B, CHUNK):
        hi = min(lo + CHUNK, B)
        g_, o_ = grad[lo:hi], np.asarray(outputs[lo:hi])
        want = freq_backward_model(g_, o_, D, deg, np.float64)
        err32 = max(err32, float(np.abs(freq_backward_model(g_, o_, D, deg, np.float32) - want).max()))
        scale = max(scale, float(np.abs(want).max()))
        g = got[lo:hi].astype(np.float64)
        with np.errstate(invalid='ignore'):
            e = max(e, float(np.where(np.isfinite(g), np.abs(g - want), np.inf).max()))
        n_diff += int((g != want).sum())
    bound = 4.0 * err32 + 1e-7 * scale          # (`whole_yardstick`, its two maxima gathered chunk by chunk)
    rep.add('grad_inputs', e <= bound, e, f'{bound:.2e}', f'float32 model error {err32:.2e}')
    if deg == 0:
        rep.add('grad_inputs is a copy', n_diff == 0, n_diff, 'exact')
    _guard(rep, 'grad_inputs', got, B, 'f32')
    return rep
