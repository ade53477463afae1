"""Cases, references and criteria shared by tests/test_optim_cases.py (CPU) and tests/test_gpu_optim_model.py (GPU): the optimizer kernels of
csrc/optim.hip -- k_check_finite, k_adam (wide path, pair loop, odd tail), k_update_scale, k_adam_small_commit (small-tensor loop, table-prefix
sweep, the ticket), k_poison_shards, k_shard_verdict -- with the Adam arithmetic they share through csrc/common.h (adam_consts, adam_element),
against a float64 model of PyTorch's Adam (amsgrad = False, weight_decay = 0) behind GradScaler's unscale / skip / update.  numpy only.

MODELS
    adam_step(dtype)   one step of one tensor.  np.float64: the DEFINITION.  np.float32: the TWIN -- every operation rounded to fp32 in the
                       order of adam_consts, adam_element and adam_group: inv_scale = grad_mult / scale, g = x * inv_scale,
                       m = b1 m + (1 - b1) g, v = b2 v + ((1 - b2) g) g, step_size = (lr lr_mult) / bc1, p -= (step_size m) / (sqrt(v) /
                       bc2_sqrt + eps), the fp16 shadow half(p_new), the EMA e - omd (e - p_new).  The betas, eps, lr, grad_mult, omd and the
                       state words enter BOTH as the float32 values the kernels receive (1 - float32(0.99), not 0.01); fp16 gradients as their
                       exact values.  `skip` (found_inf != 0, or 1 / scale not finite IN FP32) is decided in fp32 in both.
                       The twin's pow(beta, t) is the float64 power rounded once to fp32.
    commit             update_scale: all of its arithmetic (x 2, x 0.5, x 1.5, + 1) is exact in fp32 on the rows of COMMIT_TABLE or rounds
                       once (a back-off out of the smallest denormal): the model is bit-exact.  The dead-scale rows (a scale whose 1 / scale
                       overflows counts as an overflow; the sticky OPT_SCALE_DEAD word) are this project's extension of GradScaler.
    check_finite, poison_shards, shard_verdict: exact.

CRITERIA (coded once here: `step_criteria`, `state_criteria`, `same_bits`; applied by the CPU test to the twin and to the wrong variants and by
the GPU test to the kernels)
    m, v               bit for bit the twin.  They are IEEE multiplies and adds of exactly converted inputs, inv_scale is one fp32 division, and
                       the library is built with -ffp-contract=off -fno-fast-math (csrc/Makefile).  test_optim_cases shows the twin within
                       4 fp32 ulp (of the operands' magnitude |b m| + |(1 - b) g^k|) of the definition.
    p, shadow          depend on the device's powf, sqrtf and division as well.  FINDINGS:
                         divide, sqrt  correctly rounded.  `hipcc --help` lists -fhip-fp32-correctly-rounded-divide-sqrt / -fno-hip-fp32-...
                                       ("single precision floating-point divide and sqrt used in the program source are correctly rounded",
                                       HIP device compilation); the Makefile passes neither, and a two-line kernel compiled to LLVM IR with the
                                       Makefile's flags carries `fdiv float` and `llvm.sqrt.f32` WITHOUT the `!fpmath` accuracy metadata that
                                       the -fno- form attaches to both: the default is the correctly rounded expansion.  No denormal-flushing
                                       function attribute either.  The twin's np.float32 divide and sqrt are therefore the device's.
                         powf          no accuracy is stated anywhere in the toolchain's headers, help text or documents (the OCML sources and
                                       their table of ulp bounds are not shipped; __clang_hip_math.h maps powf to __ocml_pow_f32 without a
                                       figure).  MEASURED instead, kernel-independent: powf(float32(beta), t) on an MI355X for beta = 0.9 and
                                       0.99 and EVERY t = 1 .. 30016 (this covers the t of every case here) against np.power in float64 --
                                       once by torch.pow on float32 tensors (tensor ** tensor and scalar ** tensor) and once by a ten-line
                                       HIP program built with the Makefile's flags.  All three agree to the digit: the largest relative
                                       error is 1.2199e-07 (1.02 ulp; beta = 0.99, t = 7102; 1.0417e-07 for beta = 0.9), powf(beta, 1) is
                                       beta exactly, 0.9^1000 and 0.99^30000 come out as 0, and where the power is subnormal the largest
                                       absolute error is 1.47e-45 (one denormal step).  POWF_REL_ERR = 2 x 1.22e-07 (the 2 x margin), plus
                                       3 fp32 denormal steps absolute (2 x 1.47e-45, rounded up to whole steps).
                       BOUND = an envelope + a yardstick.  Envelope: the definition's update step_size m / (sqrt(v) / bc2_sqrt + eps) evaluated
                       with pow(b1, t) x (1 +- POWF_REL_ERR) and pow(b2, t) x (1 -+ POWF_REL_ERR): the update is monotone in both powers
                       (bc1 shrinks as pow(b1, t) grows: a larger step; bc2_sqrt shrinks as pow(b2, t) grows: a larger denominator), so
                       the two opposite corners bracket it.  Yardstick (the rule of network_cases.yardstick for products that span many
                       binades): 4 x the largest error of the twin's update against the definition's, RELATIVE to the magnitude
                       A = step_size (|b1 m| + |(1 - b1) g|) / denominator of the update's operands (relative to the update itself it would
                       measure the cancellation of m against g in ONE unlucky element, not the arithmetic), times A element by element, plus
                       4 fp32 denormal steps.  p_new must lie between the fp32 roundings of p - (update -/+ bound), the shadow between the fp16
                       roundings of the same two values; and the shadow must be half(stored p_new) exactly.
    EMA                evaluated from the STORED updated parameter (teacher forcing, as in network_cases: one ulp in p does not widen it):
                       4 x max |twin - definition| of the value before the fp32 store + 1e-7 x max |reference|; the output between the fp32
                       roundings of (definition -/+ bound).
    state words, the gradient zeroed (+0) or kept, check_finite, the poison and verdict buffers: exact, compared as bits (a NaN by class: the
                       poison is "a NaN", its payload is nobody's contract).  A skipped step leaves p, m, v and the shadow bitwise unchanged,
                       and with the keep bit (grad_is_half & 2) the gradient as well.

WRONG_VARIANTS are deliberately wrong models (the twin / the exact models with ONE statement changed); test_optim_cases shows that each fails
a named criterion on the cases below (REJECTED_BY there is the variant-to-case table).

CASES
    elements()         the fixture of test_gpu_optim_paths.py restated in numpy (N = 4104 = 1026 four-element groups: two trips of the wide
                       loop; N - 1 for the pair loop's odd tail; fp16 zeros, subnormals, values at 65504), plus rows with v = 0, g = 0,
                       m = +-k 1e-17 (the only rows that see eps: step_size m / eps ~ 1e-4 .. 5e-3), rows with v = {0.25, 1, 4, 100} eps^2,
                       rows with m and g of opposite sign, and for the fp32-gradient path values an fp16 cannot hold.
    STEPS              0, 1, 9, 999, 29999 in the state word (t = step + 1; 0.9^1000 and 0.99^30000 underflow to 0 in fp32)
    SCALARS            scale {128, 65536, 3 x 2^10} x lr_mult {1, 0.37} x grad_mult {1, 1/3}, four combinations that hold every value
    PATHS              wide | pair (N - 1, one element into the allocation) | g32 (fp32 gradient, no shadow) | ema (pair loop, EMA) | small |
                       prefix0 | prefix1 (table prefix read from set `parity`, written to the other)
    COMMIT_TABLE       hand-written (state in, growth, backoff, interval, flip) -> state out
    check_tensors / check_plants: eight tensors in one call, one non-finite value at a time; ALIGNMENT: optim.py hands CHECK slices of its flat fp16 buffers whose offsets are multiples of 8
                       elements -- 16 bytes, what the kernel's 8-wide loads need -- and fp32 gradients that are allocations of their own;
                       the cases do the same, no CHECK case uses a pointer less aligned than that.  With the launch grid of
                       ngp_optim_adam_step_ex (one lane per ~8 elements of the call) the 8-wide fp16 body never takes a second grid-stride
                       trip; the fp32 branch (one element per lane and trip) does, so the second-trip plant sits in an fp32 tensor.
    shard_cases / verdict_cases: shards {1, 2, 64, 65} (the launches have 64 lanes) x payload {1, 8, 1000} x found_inf {0, 1}; the verdict with
                       and without the flat pointer, element 0 of the own shard finite, NaN, +inf, -inf, poison in the other shards
    TRAJECTORY_*, TICKET_*: three steps in a row (standing, overflow, standing; interval 1: the scale changes every time); the ticket at the
                       192 + 32 workgroups the closing launch is capped at
NOT TESTED: the step counter is a float; t + 1 stops counting at 2^24 steps."""
import functools

import numpy as np

F32, F16 = np.float32, np.float16
SCALE, TRACKER, FOUND_INF, STEP, LR_MULT, PARITY, TICKET, DEAD = range(8)
WORDS = ('scale', 'tracker', 'found_inf', 'step', 'lr_mult', 'parity', 'ticket', 'dead')
F32_TINY = 2.0 ** -149

# measured (see the header): the largest relative error of the device's powf(beta, t) over beta in {0.9, 0.99}, t = 1 .. 30016
POWF_MEASURED_REL_ERR = 1.22e-7
POWF_REL_ERR = 2.0 * POWF_MEASURED_REL_ERR

WRONG_VARIANTS = ('eps inside the bias correction', 'bc2 not square-rooted', 'corrections from t', 'bias correction of m dropped',
                  'grad_mult dropped', 'lr_mult dropped', 'unscale after squaring', 'shadow from the old parameter',
                  'EMA on the parameter before the update', 'EMA not moved on a skipped step', 'step counted on a skipped step',
                  'found_inf not cleared', 'growth at tracker + 1 > interval', 'growth to inf applied', 'parity flipped on a skipped step',
                  'dead cleared once the scale is finite again', 'dead scale not an overflow in UPDATE', 'poison only in shards with a gradient',
                  'verdict cleans only its own shard')

BETA1, BETA2, EPS = F32(0.9), F32(0.99), F32(1e-15)
LRS = (F32(1e-2), F32(3e-4))          # two tensors of one call
EMA_OMD = F32(0.05)
GROWTH, BACKOFF, INTERVAL = F32(2.0), F32(0.5), F32(2000.0)

N = 4104
STEPS = (0, 1, 9, 999, 29999)
SCALARS = {'s128': dict(scale=128.0, lr_mult=1.0, grad_mult=1.0), 's65536_m.37_g3': dict(scale=65536.0, lr_mult=0.37, grad_mult=1.0 / 3.0),
           's3072_g3': dict(scale=3072.0, lr_mult=1.0, grad_mult=1.0 / 3.0), 's3072_m.37': dict(scale=3072.0, lr_mult=0.37, grad_mult=1.0)}
# path -> (n, fp32 gradient, shadow, ema, one element into the allocation)
PATHS = {'wide': (N, False, True, False, False), 'pair': (N - 1, False, True, False, True), 'g32': (N, True, False, False, False),
         'ema': (N, False, True, True, False), 'small': (N, False, True, False, False), 'prefix0': (N, False, True, False, False),
         'prefix1': (N, False, True, False, False)}
SKIPS = {'found_inf': dict(scale=128.0, found_inf=1.0), 'found_inf=3': dict(scale=3072.0, found_inf=3.0),
         'scale 0': dict(scale=0.0, found_inf=0.0), 'scale 2^-130': dict(scale=2.0 ** -130, found_inf=0.0)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    """-> number of entries whose bits differ (a NaN matches any NaN)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return int(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())


class Report(list):
    """rows (name, ok, figure, bar, note)"""
    def add(self, name, ok, figure, bar, note=''):
        self.append((name, bool(ok), figure, bar, note))

    def failures(self):
        return [r for r in self if not r[1]]

    def failed(self):
        return {r[0] for r in self if not r[1]}

    def __str__(self):
        return '\n'.join(f'{"ok  " if ok else "FAIL"} {name:22s} {fig!s:>24s}  bar {bar!s:<22s} {note}' for name, ok, fig, bar, note in self)


# ------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------
def scale_is_dead(scale):
    """1 / scale not finite in fp32: 0, and the denormals below 2^-128 (1 / 2^-127 = 2^127 is still finite)"""
    with np.errstate(all='ignore'):
        return not np.isfinite(F32(1.0) / F32(scale))


def make_state(scale=128.0, tracker=0.0, found_inf=0.0, step=3.0, lr_mult=1.0, parity=0.0, ticket=0.0, dead=0.0):
    return np.array([scale, tracker, found_inf, step, lr_mult, parity, ticket, dead], F32)


def make_rule(grad_mult=1.0, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL, beta1=BETA1, beta2=BETA2, eps=EPS):
    return dict(beta1=F32(beta1), beta2=F32(beta2), eps=F32(eps), grad_mult=F32(grad_mult), growth=F32(growth), backoff=F32(backoff),
                interval=F32(interval))


def _pow(beta, t, f, rel=0.0):
    """pow(beta, t) at `f`: float64 exactly (times 1 + rel, -/+ 3 fp32 denormal steps: the envelope's corners); float32: rounded once"""
    with np.errstate(under='ignore'):
        e = np.power(np.float64(beta), np.float64(t))
        if f == np.float64:
            return max(e * (1.0 + rel) + np.sign(rel) * 3.0 * F32_TINY, 0.0)
        return F32(e)


def adam_step(el, state, rule, lr, flags=1, omd=None, dtype=np.float64, variant=None, pow_rel=(0.0, 0.0)):
    """one UPDATE of one tensor.  el: p, m, v (float32), g (float16 or float32: the loss-scaled gradient), p16 (float16: the shadow before the
    step, optional), e (float32: the EMA shadow, with `omd`).  flags: grad_is_half (bit 1: keep the gradient).
    -> dict: skip, m, v, p (at `dtype`), upd (the update), mag (the magnitude A of the update's operands), p16 (float16), g (the gradient buffer
    afterwards), ema / ema_pre (at dtype / float64: the value before the store)"""
    f = dtype
    st = np.asarray(state, F32)
    x, m0, v0, p0 = (np.asarray(el[k]).astype(f) for k in ('g', 'm', 'v', 'p'))
    b1, b2, eps, one = f(rule['beta1']), f(rule['beta2']), f(rule['eps']), f(1.0)
    dead = scale_is_dead(st[SCALE])
    skip = bool(st[FOUND_INF] != 0) or (dead and variant != 'dead scale not an overflow in UPDATE')
    out = dict(skip=skip, g=np.array(el['g'], copy=True) if flags & 2 else np.zeros_like(el['g']))
    with np.errstate(all='ignore'):
        if skip:
            out.update(m=m0, v=v0, p=p0, upd=np.zeros_like(p0), mag=np.zeros_like(p0), p16=None if el.get('p16') is None else np.array(el['p16'], copy=True))
        else:
            inv_scale = (one if variant == 'grad_mult dropped' else f(rule['grad_mult'])) / f(st[SCALE])
            t = f(st[STEP]) + (f(0.0) if variant == 'corrections from t' else one)
            bc1 = one - f(_pow(b1, t, f, pow_rel[0]))
            bc2 = one - f(_pow(b2, t, f, pow_rel[1]))
            bc2_sqrt = bc2 if variant == 'bc2 not square-rooted' else np.sqrt(bc2)
            lr_mult = one if variant == 'lr_mult dropped' else f(st[LR_MULT])
            step_size = f(lr) * lr_mult / (one if variant == 'bias correction of m dropped' else bc1)
            g = x * inv_scale
            ma, mb = b1 * m0, (one - b1) * g
            m = ma + mb
            gv = x if variant == 'unscale after squaring' else g
            v = b2 * v0 + (one - b2) * gv * gv
            den = (np.sqrt(v) + eps) / bc2_sqrt if variant == 'eps inside the bias correction' else np.sqrt(v) / bc2_sqrt + eps
            upd = step_size * m / den
            p = p0 - upd
            assert all(a.dtype == f for a in (m, v, upd, p)), [a.dtype for a in (m, v, upd, p)]
            shadow = p0 if variant == 'shadow from the old parameter' else p
            out.update(m=m, v=v, p=p, upd=upd, mag=np.abs(step_size) * (np.abs(ma) + np.abs(mb)) / den, p16=shadow.astype(F16))
        if omd is not None:
            e0 = np.asarray(el['e']).astype(f)
            toward = p0 if (skip or variant == 'EMA on the parameter before the update') else out['p']
            move = f(omd) * (e0 - toward)
            if skip and variant == 'EMA not moved on a skipped step':
                move = np.zeros_like(e0)
            out.update(ema=e0 - move, ema_pre=e0.astype(np.float64) - move.astype(np.float64))
    return out


def commit(state, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL, flip=0, variant=None):
    """update_scale on the eight words -> the eight words (float32).  The ticket word is not update_scale's: 0 in, 0 out."""
    s = np.array(state, F32)
    assert s[TICKET] == 0
    scale, tracker, t, parity, dead = s[SCALE], s[TRACKER], s[STEP], s[PARITY], s[DEAD]
    flipped = F32(0.0) if parity != 0 else F32(1.0)
    sd = scale_is_dead(scale)
    with np.errstate(all='ignore'):
        if s[FOUND_INF] != 0 or sd:
            if sd:
                dead = F32(1.0)
            scale = F32(scale * F32(backoff))
            tracker = F32(0.0)
            if variant == 'step counted on a skipped step':
                t = F32(t + F32(1.0))
            if variant == 'parity flipped on a skipped step' and flip:
                parity = flipped
        else:
            t = F32(t + F32(1.0))
            tr = F32(tracker + F32(1.0))
            if (tr > F32(interval)) if variant == 'growth at tracker + 1 > interval' else (tr >= F32(interval)):
                grown = F32(scale * F32(growth))
                if np.isfinite(grown) or variant == 'growth to inf applied':
                    scale = grown
                tracker = F32(0.0)
            else:
                tracker = tr
            if flip:
                parity = flipped
    if variant == 'dead cleared once the scale is finite again':
        dead = F32(1.0 if sd else 0.0)
    found = s[FOUND_INF] if variant == 'found_inf not cleared' else F32(0.0)
    return np.array([scale, tracker, found, t, s[LR_MULT], parity, 0.0, dead], F32)


def check_finite(tensors, state):
    """CHECK: found_inf = 1 when any element of any tensor is not finite; every other word (and a clean found_inf) as it was"""
    out = np.array(state, F32)
    if any(not np.isfinite(np.asarray(t, np.float64)).all() for t in tensors):
        out[FOUND_INF] = 1.0
    return out


def poison_shards(flat, shards, payload, state, variant=None):
    """-> the flat fp16 gradient afterwards: NaN in element r * payload of EVERY shard r < shards when found_inf is set, untouched otherwise"""
    out = np.array(flat, F16, copy=True)
    if np.asarray(state, F32)[FOUND_INF] != 0:
        for r in range(shards):
            if variant == 'poison only in shards with a gradient' and not out[r * payload:(r + 1) * payload].any():
                continue
            out[r * payload] = np.nan
    return out


def shard_verdict(shard, state, flat, shards, payload, variant=None, rank=0):
    """-> (state afterwards, flat afterwards or None): found_inf = 1 when element 0 of the own (averaged) shard is not finite; with `flat`, a
    non-finite first element of EVERY shard of it becomes +0 (`rank` only tells the wrong variant which shard is its own)"""
    st = np.array(state, F32)
    if not np.isfinite(np.float64(np.asarray(shard)[0])):
        st[FOUND_INF] = 1.0
    if flat is None:
        return st, None
    out = np.array(flat, F16, copy=True)
    for r in range(shards):
        if variant == 'verdict cleans only its own shard' and r != rank:
            continue
        if not np.isfinite(np.float64(out[r * payload])):
            out[r * payload] = 0.0
    return st, out


# ------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------
def _between(got, lo_val, hi_val, fmt):
    """got within [round_fmt(lo_val), round_fmt(hi_val)] -> (ok array, the worst distance from the middle of that interval in units of its
    half width: at most 1 inside)"""
    got = np.asarray(got).astype(np.float64)
    with np.errstate(all='ignore'):
        lo, hi = lo_val.astype(fmt).astype(np.float64), hi_val.astype(fmt).astype(np.float64)
        ok = (got >= lo) & (got <= hi)
        dist, half_w = np.abs(got - 0.5 * (hi + lo)), 0.5 * (hi - lo)
        off = np.where(dist == 0, 0.0, dist / np.maximum(half_w, 1e-300))
    return ok, float(np.max(np.where(np.isnan(off), np.inf, off))) if got.size else 0.0


def _exact(rep, name, got, want):
    bad = same_bits(got, want)
    rep.add(name, bad == 0, bad, 'bits')


def twin_update_error(el, state, rule, lr, flags=1):
    """the yardstick's figure: max |twin's update - definition's update| / A over the elements with A > 2^-100 -> (error, the definition, the twin)"""
    ref, tw = adam_step(el, state, rule, lr, flags, dtype=np.float64), adam_step(el, state, rule, lr, flags, dtype=np.float32)
    if ref['skip']:
        return 0.0, ref, tw
    keep = ref['mag'] > 2.0 ** -100
    err = np.abs(tw['upd'].astype(np.float64) - ref['upd'])[keep] / ref['mag'][keep]
    return (float(err.max()) if keep.any() else 0.0), ref, tw


def step_criteria(got, el, state, rule, lr, flags=1, omd=None):
    """`got`: p, m, v (float32), g (the gradient buffer afterwards), p16 (float16, if the path has a shadow), ema (float32, with `omd`) of one
    implementation of UPDATE on `el` -> Report"""
    rep = Report()
    err, ref, tw = twin_update_error(el, state, rule, lr, flags)
    p0 = np.asarray(el['p'], F32)
    _exact(rep, 'gradient', got['g'], ref['g'])
    if ref['skip']:
        _exact(rep, 'p unchanged', got['p'], p0)
        _exact(rep, 'm unchanged', got['m'], np.asarray(el['m'], F32))
        _exact(rep, 'v unchanged', got['v'], np.asarray(el['v'], F32))
        if got.get('p16') is not None:
            _exact(rep, 'shadow unchanged', got['p16'], np.asarray(el['p16'], F16))
    else:
        _exact(rep, 'm bits', got['m'], tw['m'])
        _exact(rep, 'v bits', got['v'], tw['v'])
        corners = [adam_step(el, state, rule, lr, flags, pow_rel=(s * POWF_REL_ERR, -s * POWF_REL_ERR))['upd'] for s in (1.0, -1.0)]
        u_lo, u_hi = np.minimum(np.minimum(*corners), ref['upd']), np.maximum(np.maximum(*corners), ref['upd'])
        bound = 4.0 * err * ref['mag'] + 4.0 * F32_TINY
        lo_val, hi_val = p0.astype(np.float64) - (u_hi + bound), p0.astype(np.float64) - (u_lo - bound)
        ok, worst = _between(got['p'], lo_val, hi_val, F32)
        fin = bool(np.isfinite(np.asarray(got['p'], np.float64)).all())
        rep.add('p envelope', fin and ok.all(), round(worst, 4), f'1 (yardstick {4 * err:.2e} rel)',
                f'{int((~ok).sum())} outside; {same_bits(np.asarray(got["p"], F32), tw["p"])} of {p0.size} differ from the twin')
        if got.get('p16') is not None:
            ok, worst = _between(got['p16'], lo_val, hi_val, F16)
            rep.add('shadow envelope', ok.all(), round(worst, 4), '1 (fp16 roundings)', f'{int((~ok).sum())} outside')
            with np.errstate(all='ignore'):
                _exact(rep, 'shadow == half(p)', got['p16'], np.asarray(got['p'], F32).astype(F16))
    if omd is not None:
        e_ref, e_tw = (adam_step(el, state, rule, lr, flags, omd, f) for f in (np.float64, np.float32))
        bound = 4.0 * float(np.abs(e_tw['ema_pre'] - e_ref['ema_pre']).max()) + 1e-7 * float(np.abs(e_ref['ema_pre']).max())
        e0 = np.asarray(el['e'], np.float64)
        pre = e0 - np.float64(F32(omd)) * (e0 - np.asarray(got['p'], np.float64))       # from the STORED parameter
        ok, worst = _between(got['ema'], pre - bound, pre + bound, F32)
        rep.add('ema', ok.all(), round(worst, 4), f'1 ({bound:.2e} abs)', f'{int((~ok).sum())} outside')
    return rep


def state_criteria(got, want):
    """the eight state words, bit for bit, one row per word -> Report"""
    rep = Report()
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    for k, name in enumerate(WORDS):
        rep.add('state.' + name, same_bits(got[k:k + 1], want[k:k + 1]) == 0, float(got[k]), float(want[k]))
    return rep


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
G32_VALUES = (1e5, -3.3333333e-9, 1.0000001, -7e8, 2.5e-10, 123456.789)     # none of them an fp16 value


@functools.lru_cache(maxsize=None)
def elements():
    """-> dict of N-element arrays: p, m, v, e (float32), g (float16), g32 (float32: g, with G32_VALUES on every 41st row), p16 = half(p).
    Treat as read-only."""
    rng = np.random.default_rng(20)
    p = (rng.standard_normal(N) * 1e-2).astype(F32)
    m = (rng.standard_normal(N) * 1e-3).astype(F32)
    v = ((rng.standard_normal(N) * 1e-3) ** 2).astype(F32)
    g = (rng.standard_normal(N) * 4.0).astype(F16)                               # ordinary loss-scaled values
    e = (p + rng.standard_normal(N) * 1e-3).astype(F32)
    g[1::7] = 0.0                                                                # exact zeros
    sub = np.arange(3, N, 11)
    k = np.arange(sub.size)
    g[sub] = ((k % 1023 + 1) * 2.0 ** -24 * (1 - 2 * (k % 2))).astype(F16)       # subnormals
    big = np.arange(5, N, 13)
    g[big] = np.resize(np.array([65504.0, -65504.0, 65472.0, -65472.0, 65024.0, -64512.0], F16), big.size)
    rows = np.arange(8, N, 29)                                                   # v = 0, g = 0, m != 0: the rows that see eps
    k = np.arange(rows.size)
    g[rows], v[rows], m[rows] = 0.0, 0.0, (F32(1e-17) * (1 + k % 5) * (1 - 2 * (k % 2))).astype(F32)
    rows = np.arange(11, N, 31)                                                  # v around eps^2
    k = np.arange(rows.size)
    g[rows], m[rows] = 0.0, (F32(1e-16) * (1 - 2 * (k % 2))).astype(F32)
    v[rows] = (np.float64(EPS) ** 2 * np.array([0.25, 1.0, 4.0, 100.0])[k % 4]).astype(F32)
    rows = np.arange(12, N, 37)                                                  # m and g of opposite sign
    k = np.arange(rows.size)
    g[rows], m[rows] = (2.0 * (1 - 2 * (k % 2))).astype(F16), (-1e-3 * (1 + k % 3) * (1 - 2 * (k % 2))).astype(F32)
    g32 = g.astype(F32)
    rows = np.arange(14, N, 41)
    g32[rows] = np.resize(np.array(G32_VALUES, F32), rows.size)
    out = dict(p=p, m=m, v=v, e=e, g=g, g32=g32, p16=p.astype(F16))
    for a in out.values():
        a.setflags(write=False)
    return out


def path_elements(path, tile=1):
    """the element set as `path` takes it: the first n elements, g = the fp16 or the fp32 gradient (`tile`: repeated that many times)"""
    n, g32, shadow, ema, _ = PATHS[path]
    src = elements()
    el = {k: src[k][:n] for k in ('p', 'm', 'v', 'e')}
    el['g'] = src['g32' if g32 else 'g'][:n]
    el['p16'] = src['p16'][:n] if shadow else None
    if tile > 1:
        el = {k: (None if a is None else np.tile(a, tile)) for k, a in el.items()}
    return el


def step_case(path, step, scalars, keep=False):
    """-> dict: el, state (float32 [8]), rule, lr, flags, omd, flip -- one standing step of `path`"""
    s = SCALARS[scalars]
    return _case(path, make_state(scale=s['scale'], step=float(step), lr_mult=s['lr_mult'], parity=1.0 if path == 'prefix1' else 0.0, tracker=5.0),
                 s['grad_mult'], keep)


def skip_case(path, kind, keep=False):
    """-> the same for a step that must be skipped (SKIPS)"""
    s = SKIPS[kind]
    return _case(path, make_state(scale=s['scale'], found_inf=s['found_inf'], step=9.0, lr_mult=0.37, parity=1.0 if path == 'prefix1' else 0.0, tracker=5.0),
                 1.0 / 3.0, keep)


def _case(path, state, grad_mult, keep):
    n, g32, shadow, ema, offset = PATHS[path]
    prefix = path.startswith('prefix')        # (its gradient is the table's stored one: read, never written -- the keep bit says that to the model)
    return dict(path=path, el=path_elements(path), state=state, rule=make_rule(grad_mult), lr=LRS[0], flags=(0 if g32 else 1) | (2 if keep or prefix else 0),
                omd=EMA_OMD if ema else None, flip=1 if prefix else 0, offset=offset)


def run_model(case, dtype=np.float32, variant=None):
    """an implementation of a case: what the launch leaves behind (float32 / float16 arrays) -> (got for step_criteria, state afterwards for
    the paths whose launch also commits, else the state unchanged)"""
    r = adam_step(case['el'], case['state'], case['rule'], case['lr'], case['flags'], case['omd'], dtype, variant)
    with np.errstate(all='ignore'):
        got = dict(p=r['p'].astype(F32), m=r['m'].astype(F32), v=r['v'].astype(F32), g=r['g'], p16=r['p16'] if case['el']['p16'] is not None else None)
        if case['omd'] is not None:
            got['ema'] = r['ema'].astype(F32)
    if case['path'] in ('small', 'prefix0', 'prefix1'):
        rule = case['rule']
        return got, commit(case['state'], rule['growth'], rule['backoff'], rule['interval'], case['flip'], variant)
    return got, np.array(case['state'], F32)


def case_criteria(got, state_after, case):
    """every criterion of one case -> Report"""
    rep = step_criteria(got, case['el'], case['state'], case['rule'], case['lr'], case['flags'], case['omd'])
    want = run_model(case)[1]
    return Report(rep + state_criteria(state_after, want))


# (state in, growth, backoff, interval, flip) -> state out; words: scale, tracker, found_inf, step, lr_mult, parity, ticket, dead.
# `gradscaler`: torch.amp.GradScaler's update defines the row's scale and tracker (it grows at tracker + 1 == interval only, and knows no dead scale)
_T = 2.0 ** 127
COMMIT_TABLE = (
    # the tracker at interval - 2, interval - 1, interval
    dict(name='tracker I-2', state=(1024, 2, 0, 7, .37, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(1024, 3, 0, 8, .37, 0, 0, 0), gradscaler=True),
    dict(name='tracker I-1', state=(1024, 3, 0, 7, .37, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(2048, 0, 0, 8, .37, 0, 0, 0), gradscaler=True),
    dict(name='tracker I', state=(1024, 4, 0, 7, .37, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(2048, 0, 0, 8, .37, 0, 0, 0), gradscaler=False),
    dict(name='interval 1, growth 1.5', state=(3072, 0, 0, 0, 1, 0, 0, 0), rule=(1.5, .25, 1), flip=0, out=(4608, 0, 0, 1, 1, 0, 0, 0), gradscaler=True),
    dict(name='growth to inf withheld', state=(_T, 3, 0, 7, 1, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(_T, 0, 0, 8, 1, 0, 0, 0), gradscaler=True),
    dict(name='overflow', state=(1024, 2, 1, 7, .37, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(512, 0, 0, 7, .37, 0, 0, 0), gradscaler=True),
    dict(name='overflow, found_inf = 2, backoff .25', state=(3072, 3, 2, 7, 1, 0, 0, 0), rule=(2, .25, 4), flip=0, out=(768, 0, 0, 7, 1, 0, 0, 0), gradscaler=True),
    # the scale's way down
    dict(name='back-off into a denormal', state=(2.0 ** -126, 1, 1, 7, 1, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(2.0 ** -127, 0, 0, 7, 1, 0, 0, 0), gradscaler=True),
    dict(name='denormal 2^-127 is usable', state=(2.0 ** -127, 0, 0, 7, 1, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(2.0 ** -127, 1, 0, 8, 1, 0, 0, 0), gradscaler=True),
    dict(name='denormal 2^-130 is dead', state=(2.0 ** -130, 2, 0, 7, 1, 0, 0, 0), rule=(2, .5, 4), flip=1, out=(2.0 ** -131, 0, 0, 7, 1, 0, 0, 1), gradscaler=False),
    dict(name='smallest denormal to 0', state=(2.0 ** -149, 0, 1, 7, 1, 1, 0, 0), rule=(2, .5, 4), flip=1, out=(0, 0, 0, 7, 1, 1, 0, 1), gradscaler=False),
    dict(name='scale 0', state=(0, 3, 0, 7, 1, 0, 0, 0), rule=(2, .5, 4), flip=0, out=(0, 0, 0, 7, 1, 0, 0, 1), gradscaler=False),
    dict(name='scale 0, dead already', state=(0, 0, 1, 7, 1, 0, 0, 1), rule=(2, .5, 4), flip=0, out=(0, 0, 0, 7, 1, 0, 0, 1), gradscaler=False),
    dict(name='dead is sticky', state=(1024, 1, 0, 7, 1, 0, 0, 1), rule=(2, .5, 4), flip=0, out=(1024, 2, 0, 8, 1, 0, 0, 1), gradscaler=False),
    dict(name='dead is sticky on an overflow', state=(1024, 1, 1, 7, 1, 0, 0, 1), rule=(2, .5, 4), flip=0, out=(512, 0, 0, 7, 1, 0, 0, 1), gradscaler=False),
    # parity 0 / 1, with and without FLIP, standing and skipped
    dict(name='standing, parity 0, flip', state=(128, 0, 0, 3, .5, 0, 0, 0), rule=(2, .5, 2000), flip=1, out=(128, 1, 0, 4, .5, 1, 0, 0), gradscaler=True),
    dict(name='standing, parity 1, flip', state=(128, 0, 0, 3, .5, 1, 0, 0), rule=(2, .5, 2000), flip=1, out=(128, 1, 0, 4, .5, 0, 0, 0), gradscaler=True),
    dict(name='standing, parity 0', state=(128, 0, 0, 3, .5, 0, 0, 0), rule=(2, .5, 2000), flip=0, out=(128, 1, 0, 4, .5, 0, 0, 0), gradscaler=True),
    dict(name='standing, parity 1', state=(128, 0, 0, 3, .5, 1, 0, 0), rule=(2, .5, 2000), flip=0, out=(128, 1, 0, 4, .5, 1, 0, 0), gradscaler=True),
    dict(name='skipped, parity 0, flip', state=(128, 7, 1, 3, .5, 0, 0, 0), rule=(2, .5, 2000), flip=1, out=(64, 0, 0, 3, .5, 0, 0, 0), gradscaler=True),
    dict(name='skipped, parity 1, flip', state=(128, 7, 1, 3, .5, 1, 0, 0), rule=(2, .5, 2000), flip=1, out=(64, 0, 0, 3, .5, 1, 0, 0), gradscaler=True),
    dict(name='skipped, parity 0', state=(128, 7, 1, 3, .5, 0, 0, 0), rule=(2, .5, 2000), flip=0, out=(64, 0, 0, 3, .5, 0, 0, 0), gradscaler=True),
    dict(name='skipped, parity 1', state=(128, 7, 1, 3, .5, 1, 0, 0), rule=(2, .5, 2000), flip=0, out=(64, 0, 0, 3, .5, 1, 0, 0), gradscaler=True),
)


# ---- the three-step trajectory: standing (the scale grows: interval 1), overflow (backs off), standing (grows again) ----
TRAJECTORY_RULE = dict(growth=2.0, backoff=0.5, interval=1.0, grad_mult=1.0 / 3.0)
TRAJECTORY_STATE = dict(scale=3072.0, step=8.0, lr_mult=0.37)
TRAJECTORY_OVERFLOW = (False, True, False)

# ---- the ticket at the launch's largest grid: 192 prefix workgroups x 1024 lanes x 8 parameters, 32 x 1024 small-tensor elements ----
TICKET_PREFIX = 192 * 1024 * 8
TICKET_SMALL = 32 * 1024


def tiled(a, n):
    """the first n elements of `a` repeated"""
    return np.resize(np.asarray(a), n)


def ticket_elements():
    """-> (prefix el [TICKET_PREFIX], small el [TICKET_SMALL]): the element set repeated (the small tensor starts at another row)"""
    src = elements()
    pre = {k: tiled(src[k], TICKET_PREFIX) for k in ('p', 'm', 'v', 'g', 'p16')}
    small = {k: tiled(np.roll(src[k], -5), TICKET_SMALL) for k in ('p', 'm', 'v', 'g', 'p16')}
    return pre, small


# ---- CHECK ----
# (length, fp16): n % 8 in {0, 1, 7}, a tail-only tensor, one-element tensors, an fp32 tensor of more than one trip
CHECK_TENSORS = ((4104, True), (4097, True), (4103, True), (8, True), (7, True), (3001, False), (5000, False), (1, False))
CHECK_LANES = 256 * (-(-(sum(n for n, _ in CHECK_TENSORS) // 2 + 1) // 1024))      # lanes of the launch: opt_blocks(total) x OPT_THREADS
BAD = (np.inf, -np.inf, np.nan)


def check_tensors():
    """-> list of 8 arrays (float16 / float32) without a non-finite value: 65504, -65504, subnormals and ordinary values"""
    out = []
    for k, (n, is_half) in enumerate(CHECK_TENSORS):
        rng = np.random.default_rng([77, k])
        a = (rng.standard_normal(n) * 100.0).astype(F16 if is_half else F32)
        a[0::5] = 65504.0 if is_half else np.finfo(F32).max
        a[1::5] = -65504.0 if is_half else -np.finfo(F32).max
        a[2::5] = 2.0 ** -24 if is_half else 2.0 ** -149
        a[3::5] = -2.0 ** -15 if is_half else -2.0 ** -127
        out.append(a)
    return out


def check_plants():
    """-> list of (name, tensor slot, element, value): one plant at a time"""
    rows = [('first element', 2, 0), ('last of the 8-wide body', 2, 4103 // 8 * 8 - 1), ('first of the tail', 2, 4103 // 8 * 8), ('last of the tail', 2, 4102),
            ('n % 8 == 1: the one-element tail', 1, 4096), ('n % 8 == 0: the last element', 0, 4103), ('tail-only tensor', 4, 6),
            ('fp32, first element of the second trip', 6, CHECK_LANES), ('fp32, last element', 6, 4999), ('fp32, last lane of the first trip', 6, CHECK_LANES - 1)]
    rows += [(f'slot {k}', k, n // 2) for k, (n, _) in enumerate(CHECK_TENSORS)]
    assert CHECK_LANES < 5000 and all(e < CHECK_TENSORS[k][0] for _, k, e in rows)
    return [(name, k, e, BAD[i % 3]) for i, (name, k, e) in enumerate(rows)]


# ---- poison and verdict ----
SHARDS, PAYLOADS = (1, 2, 64, 65), (1, 8, 1000)
OWN_FIRST = (0.25, np.nan, np.inf, -np.inf)


def shard_pattern(shards, payload):
    """a recognisable flat fp16 buffer [shards * payload]: element i holds 1 + (i % 2039) / 8 (exact in fp16, never 0); shard 1 (if any) is
    all zeros -- a shard without a gradient gets its poison like every other"""
    flat = (1.0 + (np.arange(shards * payload) % 2039) / 8.0).astype(F16)
    if shards > 1:
        flat[payload:2 * payload] = 0.0
    return flat


def verdict_flat(shards, payload, own, rank):
    """a flat buffer as it is after the exchange on a rank that poisoned: NaN in element 0 of every shard but `rank`, whose element 0 is `own`;
    with more than two shards one other shard holds -inf and one a finite value (the cleaning looks at the value, not at who wrote it)"""
    flat = shard_pattern(shards, payload)
    flat[::payload] = np.nan
    flat[rank * payload] = own
    if shards > 2:
        flat[(rank + 1) % shards * payload] = -np.inf
        flat[(rank + 2) % shards * payload] = 3.5
    return flat


def shard_cases():
    """-> list of (shards, payload, found_inf)"""
    return [(s, p, f) for s in SHARDS for p in PAYLOADS for f in (0.0, 1.0)]


def verdict_cases():
    """-> list of (shards, payload, own first element, with the flat pointer, rank): the last rank of the layout, and rank 0"""
    return [(s, p, own, with_flat, rank) for s in SHARDS for p in PAYLOADS for own in OWN_FIRST for with_flat in (False, True)
            for rank in sorted({0, s - 1})]


def poison_criteria(got_flat, flat, shards, payload, state):
    rep = Report()
    _exact(rep, 'poison buffer', got_flat, poison_shards(flat, shards, payload, state))
    return rep


def verdict_criteria(got_state, got_flat, shard, state, flat, shards, payload, with_flat):
    """got_flat: the flat buffer `flat` afterwards (with_flat False: the call did not get it, and it must be as it was)"""
    want_state, want_flat = shard_verdict(shard, state, flat if with_flat else None, shards, payload)
    rep = state_criteria(got_state, want_state)
    _exact(rep, 'verdict flat', got_flat, want_flat if with_flat else flat)
    return Report([(('verdict ' + r[0]) if r[0].startswith('state.') else r[0],) + r[1:] for r in rep])


def own_shard(payload, own):
    """the averaged shard a rank holds after the exchange: `own` in element 0, ordinary values behind it"""
    shard = (0.5 + np.arange(payload) / 16.0).astype(F16)
    shard[0] = own
    return shard
