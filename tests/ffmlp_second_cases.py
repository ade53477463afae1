"""Case table and float64 reference for the FFMLP second-order tests (tests/test_ffmlp_second_order.py on the CPU,
tests/test_gpu_ffmlp_second_order.py on the GPU).  numpy + oracle only: nothing here touches a GPU.

The second order differentiates the first backward AS IMPLEMENTED (oracle.ffmlp_backward: the activation derivative is f(h), a function
of the stored post-activation h) with respect to everything grad_inputs depends on, given u = d loss / d grad_inputs:
  tangent   p_0 = u;  q_l = p_{l-1} W_{l-1}^T,  p_l = q_l f(h_l);  d loss / d g = p_n W_n^T
  explicit  d loss / d W_l += d_{l+1}^T p_l (l < n),  d loss / d W_n = g^T p_n
  implicit  (f' != 0)  r_l = q_l e_l f'(h_l);  t_n = r_n;  s_l = t_l f(h_l);  d loss / d W_{l-1} += s_l^T h_{l-1};
            t_{l-1} = s_l W_{l-1} (+ r_{l-1});  d loss / d x = t_0

Rounding points (`round_points=True`): exactly the intermediates the kernels store as fp16 --
  d_l = e_l f(h_l)         the hidden gradients of the first backward, recomputed by the entry
  p_l = q_l f(h_l)         the tangents (the product of the UNROUNDED q_l)
  q_l                      rounded where the implicit terms read it back (r_l); activations with f' != 0 only
  s_l = t_l f(h_l)
h_l is the fp16 forward buffer in either mode; e_l, r_l, t_l never cross memory and stay unrounded.  The outputs are compared as the
float64 values (the kernels round them to fp16 once).

Inputs follow tests/ffmlp_act_cases.py (fp16-representable x and w, weight_scale 0.5 for Exp).  g and u are scaled by powers of two chosen
from the UNROUNDED reference alone: d loss / d g is linear in u, d loss / d x is linear in u and in g, so 2^ku puts max |d loss / d g| into
(1/4, 1/2] and then 2^kg puts max |d loss / d x| there (f' = 0: kg puts the first backward's max |dL/dx| there, as ffmlp_act_cases does).

Replacements: none -- every listed case meets check_conditions (tests/test_ffmlp_second_order.py runs it over the whole table).
Raised bars: none (EXTRA_BARS is empty; a case may only be listed there with at most twice its rounding sensitivity)."""
import functools

import numpy as np

import oracle

import ffmlp_act_cases as A

ACT_NAMES = A.ACT_NAMES
SLOPED = (1, 3, 4, 5)      # activations with f' != 0: Exp, Sigmoid, Squareplus, Softplus
BATCHES = A.BATCHES        # 128: one workgroup, one slab per term | 4224: 33 workgroups, 17 sample chunks per term
DX_TOL, W_L2, W_MAX = A.DX_TOL, A.W_L2, A.W_MAX

ALL_ACT_SHAPE = (32, 64, 3)
SHAPES = [(32, 16, 2), (16, 32, 3), (48, 64, 3), (96, 64, 2), (32, 128, 2), (48, 256, 3), (32, 64, 5)]
CASES = [ALL_ACT_SHAPE + (a,) for a in range(7)] + [s + (a,) for s in SHAPES for a in (5, 6)]

# (din, hid, nl, act, B) -> {'dg' | 'dx' | 'w': bar}: a bar above the constants, at most twice that case's rounding sensitivity
EXTRA_BARS = {}

MODULE_CASE = (32, 64, 3, 5)   # FFMLP(32, 1, 64, 3, 'softplus')
MODULE_B = 256


def r16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def f_of(h, act):
    """the first backward's factor as a function of the stored post-activation"""
    return (h > 0).astype(np.float64) if act == 0 else oracle._act_backward_factor(h, act)


def f_prime(h, act):
    if act == 1:
        return np.ones_like(h)
    if act == 3:
        return 1.0 - 2.0 * h
    if act == 4:
        s = 10.0 * h
        return 20.0 * s / (s * s + 1.0) ** 2
    if act == 5:
        return 10.0 * np.exp(-10.0 * h)
    return np.zeros_like(h)


def reference(g, x, w, fb, u, din, hid, nl, act, round_points):
    """-> dict(dg [B,16], dx [B,din], gw flat, and the stored intermediates d, p, q, s as lists); float64 throughout"""
    rp = r16 if round_points else (lambda a: a)
    mats = [np.asarray(m, np.float64) for m in oracle.ffmlp_split_weights(w, din, 16, hid, nl)]
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    h = [np.asarray(x, np.float64)] + [np.asarray(fb[l], np.float64) for l in range(nl)]
    e, d = [None] * (nl + 1), [None] * (nl + 1)
    e[nl] = g @ mats[nl]
    for l in range(nl, 0, -1):
        d[l] = rp(e[l] * f_of(h[l], act))
        e[l - 1] = d[l] @ mats[l - 1]
    p, q = [u], [None]
    for l in range(1, nl + 1):
        ql = p[l - 1] @ mats[l - 1].T
        p.append(rp(ql * f_of(h[l], act)))
        q.append(rp(ql))
    dg = p[nl] @ mats[nl].T
    gws = [d[l + 1].T @ p[l] for l in range(nl)] + [g.T @ p[nl]]
    s = [None] * (nl + 1)
    dx = np.zeros_like(h[0])
    if act in SLOPED:
        t = None
        for l in range(nl, 0, -1):
            r = q[l] * e[l] * f_prime(h[l], act)
            t = r if t is None else t + r
            s[l] = rp(t * f_of(h[l], act))
            gws[l - 1] = gws[l - 1] + s[l].T @ h[l - 1]
            t = s[l] @ mats[l - 1]
        dx = t
    return dict(dg=dg, dx=dx, gw=np.concatenate([m.reshape(-1) for m in gws]), d=d[1:], p=p[1:], q=q[1:], s=s[1:])


def _pow2_into_half(m):
    """k with m 2^k in (1/4, 1/2]: the middle of [2^-3, 1]"""
    return int(np.floor(np.log2(0.5 / m))) if np.isfinite(m) and m > 0 else 0


@functools.lru_cache(maxsize=4)
def case(din, hid, nl, act, B):
    """inputs, the scaled g and u, and every reference value of one case.  Shared between the tests that ask for the same case; read-only."""
    rng, x, w = A._inputs(din, hid, nl, act, B)
    _, rfb = oracle.ffmlp_forward(x, w, din, 16, hid, nl, activation=act)
    g0, u0 = rng.normal(size=(B, 16)), rng.normal(size=(B, din))
    # power-of-two scales from the unrounded reference alone
    r0 = reference(g0, x, w, rfb, u0, din, hid, nl, act, False)
    ku = _pow2_into_half(np.abs(r0['dg']).max())
    if act in SLOPED:
        kg = _pow2_into_half(np.abs(r0['dx']).max() * 2.0 ** ku)
    else:
        gx0, _ = oracle.ffmlp_backward(g0, x, w, rfb, din, 16, hid, nl, round_hidden=False, activation=act)
        kg = _pow2_into_half(np.abs(gx0).max())
    g, u = oracle.round_fp16(g0 * 2.0 ** kg), oracle.round_fp16(u0 * 2.0 ** ku)
    ref = reference(g, x, w, rfb, u, din, hid, nl, act, True)
    exact = reference(g, x, w, rfb, u, din, hid, nl, act, False)
    # rounding sensitivity: the distance between the reference with and without its rounding points, in the units of each bar
    with np.errstate(invalid='ignore', divide='ignore'):
        sens = dict(dg=A.dx_errors(ref['dg'], exact['dg'])[0],
                    dx=A.dx_errors(ref['dx'], exact['dx'])[0] if act in SLOPED else 0.0,
                    w=max(max(e) for e in A.w_errors(ref['gw'], exact['gw'], din, hid, nl)))
    c = dict(x=x, w=w, g=g, u=u, kg=kg, ku=ku, rfb=rfb, dg=ref['dg'], dx=ref['dx'], gw=ref['gw'], sens=sens,
             stored=[np.stack(ref[k], 0) for k in ('d', 'p') + (('q', 's') if act in SLOPED else ())])
    for v in list(c.values()) + c['stored']:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_conditions(c, din, hid, nl, act):
    """Conditions every case must meet -- on the REFERENCE, never on what a kernel returned: every fp16-rounded value finite and below
    2^15; max |dL/dg| in [2^-3, 1] and, where f' != 0, max |dL/dx| in [2^-3, 1]; at most 2 % of the non-zero reference dL/dx and dL/dg
    entries below the smallest normal fp16 number; every weight-gradient matrix non-zero."""
    for name, v in [(k, c[k]) for k in ('x', 'w', 'g', 'u', 'rfb', 'dg', 'dx', 'gw')] + [('stored', s) for s in c['stored']]:
        assert np.isfinite(v).all() and np.abs(v).max() < 2.0 ** 15, (name, float(np.abs(v).max()))
    for name in ('dg', 'dx'):
        a = np.abs(c[name])
        if name == 'dx' and act not in SLOPED:
            assert a.max() == 0.0
            continue
        assert 2.0 ** -3 <= a.max() <= 1.0, (name, float(a.max()))
        nz = a[a > 0]
        assert nz.size > 0.5 * a.size, name
        assert (nz < 2.0 ** -14).mean() <= 0.02, (name, float((nz < 2.0 ** -14).mean()))
    for m in A.split(c['gw'], din, hid, nl):
        assert np.abs(m).max() > 0
    assert all(np.isfinite(v) for v in c['sens'].values())


def bars(din, hid, nl, act, B):
    """(dg, dx, w L2, w max) bars of a case: the constants of tests/ffmlp_act_cases.py unless EXTRA_BARS lists the case"""
    extra = EXTRA_BARS.get((din, hid, nl, act, B), {})
    return (extra.get('dg', DX_TOL), extra.get('dx', DX_TOL), extra.get('w', W_L2), extra.get('w', W_MAX))
