"""Case table and reference data for the FFMLP activation tests (tests/test_ffmlp_activations.py on the CPU,
tests/test_gpu_ffmlp.py on the GPU).  numpy + oracle only: nothing here touches a GPU.

Activation ids: 0 ReLU, 1 Exp, 2 Sine, 3 Sigmoid, 4 Squareplus, 5 Softplus, 6 None.

Why the data is not the usual x ~ U(-1,1), w ~ U(-1,1) sqrt(3/hid), g ~ 0.1 N(0,1):
  * Exp overflows fp16 at weight scale 1.0 on the deeper nets: its weights are halved.
  * Sigmoid / Squareplus / Softplus shrink dL/dx towards the fp16 subnormals as depth grows, and a subnormal gradient compares
    nothing.  The output gradient of every case is therefore scaled by a power of two chosen FROM THE ORACLE ALONE (the
    unrounded float64 backward, which is linear in g) so that max |dL/dx| lands in [2^-3, 1].
`check_conditions` states what every case must then satisfy; it runs on the CPU over the whole table and again at the top of
every GPU test, so that a vacuous case fails instead of passing."""
import functools

import numpy as np

import oracle

ACT_NAMES = {0: 'relu', 1: 'exp', 2: 'sine', 3: 'sigmoid', 4: 'squareplus', 5: 'softplus', 6: 'none'}
SMOOTH = (1, 2, 3, 4, 5, 6)
BATCHES = (128, 4224)   # 4 tiles: one workgroup, direct weight-gradient store | 132 tiles: 33 workgroups, fp32 slabs + reduction


def weight_scale(act):
    return 0.5 if act == 1 else 1.0


# ---- (a) register-resident backward: every (W, IN_JB, NHM) instantiation of k_ffmlp_backward_paired<.., false> (NHM 1, 2) and
# k_ffmlp_backward<.., 3, false>; in_dim 48 / 16 are not multiples of 32; 64 -> 64 x 4 is the single-stage-buffer case (pf_depth 1)
FAST_SHAPES = [  # din, hid, nl            kernel reached with activation != 0
    (32, 64, 2),   # k_ffmlp_backward_paired<64, 1, 1, false>
    (32, 64, 3),   # k_ffmlp_backward_paired<64, 1, 2, false>
    (32, 64, 4),   # k_ffmlp_backward<64, 1, 3, false>
    (64, 64, 2),   # k_ffmlp_backward_paired<64, 2, 1, false>
    (48, 64, 3),   # k_ffmlp_backward_paired<64, 2, 2, false>
    (64, 64, 4),   # k_ffmlp_backward<64, 2, 3, false>, pf_depth 1
    (32, 32, 2),   # k_ffmlp_backward_paired<32, 1, 1, false>
    (16, 32, 3),   # k_ffmlp_backward_paired<32, 1, 2, false>
    (32, 32, 4),   # k_ffmlp_backward<32, 1, 3, false>
    (64, 32, 2),   # k_ffmlp_backward_paired<32, 2, 1, false>
    (64, 32, 3),   # k_ffmlp_backward_paired<32, 2, 2, false>
    (48, 32, 4),   # k_ffmlp_backward<32, 2, 3, false>
]
FAST_ALL_ACTS = [(32, 64, 2), (32, 64, 3), (64, 64, 4), (16, 32, 3)]
FAST_CASES = [(d, h, n, a) for (d, h, n) in FAST_SHAPES for a in (5, 6)] + \
             [(d, h, n, a) for (d, h, n) in FAST_ALL_ACTS for a in (1, 2, 3, 4)]

# ---- (b) NGP_FF_SINGLE_WAVE: k_ffmlp_backward<W, J, 1|2, *> on 2- and 3-layer nets; (64, 64, 3) is <64, 2, 2, *>
SINGLE_WAVE_SHAPES = [(32, 64, 2), (64, 64, 3), (32, 32, 3), (64, 32, 2)]
SINGLE_WAVE_CASES = [(d, h, n, a) for (d, h, n) in SINGLE_WAVE_SHAPES for a in (0, 5)]

# ---- (c) layered backward: k_ffmlp_dgrad_layered<W, false> for W = 16, 128, 256, 64 (96 inputs; 5 layers), and 64 again under
# NGP_FF_LAYERED; width 32 through (32, 32, 5).  flag = 1 forces NGP_FF_LAYERED on a shape the register-resident kernels would serve.
LAYERED_CASES = [  # din, hid, nl, act, flag
    (32, 16, 2, 5, 0), (32, 16, 2, 6, 0),
    (32, 128, 2, 1, 0), (32, 128, 2, 2, 0), (32, 128, 2, 3, 0), (32, 128, 2, 4, 0), (32, 128, 2, 5, 0), (32, 128, 2, 6, 0),
    (48, 256, 3, 3, 0), (48, 256, 3, 6, 0),
    (96, 64, 2, 4, 0), (96, 64, 2, 6, 0),
    (32, 64, 5, 1, 0), (32, 64, 5, 6, 0),      # more than 4 layers: Exp and None (the saturating ones run out of fp16 range with depth)
    (32, 32, 5, 1, 0), (32, 32, 5, 6, 0),
    (32, 64, 2, 3, 1), (32, 64, 2, 6, 1),
]

# ---- (d) output_activation is ignored by the backward: one register-resident and one layered shape
OUT_ACT_IGNORED_CASES = [(32, 64, 3, 3, 0), (32, 128, 2, 5, 0)]

# ---- (e) forward / inference: non-PLAIN k_ffmlp_forward<16|32|64>, k_ffmlp_forward_wide<128>, k_ffmlp_forward_layered<256>,
# the layered forward for > 64-wide images that do not fit (6 layers), > 64 inputs, and NGP_FF_LAYERED
FORWARD_SHAPES = [(32, 16, 2, 0), (16, 32, 3, 0), (32, 64, 3, 0), (32, 128, 2, 0), (32, 256, 2, 0), (32, 64, 6, 0), (96, 64, 2, 0), (32, 64, 2, 1)]
FORWARD_CASES = [(d, h, n, a, 6, f) for (d, h, n, f) in FORWARD_SHAPES for a in SMOOTH] + \
                [(d, h, 2, 0, oa, 0) for (d, h) in ((32, 64), (32, 128)) for oa in (0, 1, 2, 3, 4, 5)]

# ---- (f) module level: FFMLP(32, 3, 64, 3, activation='sigmoid'); three of the sixteen padded output columns carry a gradient
MODULE_CASE = (32, 64, 3, 3)
MODULE_OUT = 3
MODULE_B = 128


def backward_case_table():
    """every (din, hid, nl, act) any backward test uses"""
    t = set(FAST_CASES) | set(SINGLE_WAVE_CASES) | {c[:4] for c in LAYERED_CASES} | {c[:4] for c in OUT_ACT_IGNORED_CASES} | {MODULE_CASE}
    return sorted(t)


def n_params(din, hid, nl):
    return hid * (din + hid * (nl - 1) + 16)


def _inputs(din, hid, nl, act, B):
    rng = np.random.default_rng([din, hid, nl, act, B])
    w = oracle.round_fp16(rng.uniform(-1, 1, n_params(din, hid, nl)) * np.sqrt(3 / hid) * weight_scale(act))
    x = oracle.round_fp16(rng.uniform(-1, 1, (B, din)))
    return rng, x, w


@functools.lru_cache(maxsize=4)
def forward_case(din, hid, nl, act, out_act, B):
    """x, w (fp16-representable) and the oracle's outputs; the inputs do not depend on out_act"""
    _, x, w = _inputs(din, hid, nl, act, B)
    ref, rfb = oracle.ffmlp_forward(x, w, din, 16, hid, nl, activation=act, output_activation=out_act)
    c = dict(x=x, w=w, ref=ref, rfb=rfb)
    for v in c.values():
        v.setflags(write=False)
    return c


def split(gw, din, hid, nl):
    return oracle.ffmlp_split_weights(gw, din, 16, hid, nl)


@functools.lru_cache(maxsize=4)
def backward_case(din, hid, nl, act, B, out_cols=16):
    """inputs, the scaled output gradient and every reference value of one backward case.  The arrays are shared between the tests that
    ask for the same case and are read-only.  out_cols < 16: only that many output columns carry a gradient (a module whose output is
    padded to 16 columns)."""
    rng, x, w = _inputs(din, hid, nl, act, B)
    ref, rfb = oracle.ffmlp_forward(x, w, din, 16, hid, nl, activation=act)
    g0 = rng.normal(size=(B, 16))
    g0[:, out_cols:] = 0.0
    # power-of-two output-gradient scale from the oracle only: the unrounded float64 backward is linear in g
    gx0, _ = oracle.ffmlp_backward(g0, x, w, rfb, din, 16, hid, nl, round_hidden=False, activation=act)
    m = np.abs(gx0).max()
    k = int(np.floor(np.log2(0.5 / m))) if np.isfinite(m) and m > 0 else 0    # m 2^k in (1/4, 1/2]: the middle of [2^-3, 1]
    g = oracle.round_fp16(g0 * 2.0 ** k)
    rgx, rgw, hidden = oracle.ffmlp_backward(g, x, w, rfb, din, 16, hid, nl, activation=act, return_hidden=True)
    # the reference's own noise: the same computation, same rounding points, in float32
    gx32, gw32 = oracle.ffmlp_backward(g, x, w, rfb, din, 16, hid, nl, activation=act, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        floor_dx = float(np.abs(gx32 - rgx).max() / np.abs(rgx).max())
        floor_w = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(split(gw32, din, hid, nl), split(rgw, din, hid, nl))]
    c = dict(x=x, w=w, g=g, k=k, ref=ref, rfb=rfb, rgx=rgx, rgw=rgw, hidden=np.stack(hidden, 0), floor_dx=floor_dx, floor_w=floor_w)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_forward_conditions(c):
    """every value the oracle rounds to fp16 is finite and below 2^15"""
    for name in ('x', 'w', 'rfb', 'ref'):
        v = c[name]
        assert np.isfinite(v).all() and np.abs(v).max() < 2.0 ** 15, (name, float(np.abs(v).max()))


def check_conditions(c, din, hid, nl):
    """Caps every backward case must meet (they are conditions on the REFERENCE, never on what a kernel returned):
    every fp16-rounded value finite and below 2^15; max |dL/dx| in [2^-3, 1]; at most 2 % of the non-zero dL/dx entries below the
    smallest normal fp16 number; every weight-gradient matrix non-zero."""
    for name in ('x', 'w', 'g', 'rfb', 'ref', 'hidden', 'rgx'):
        v = c[name]
        assert np.isfinite(v).all() and np.abs(v).max() < 2.0 ** 15, (name, float(np.abs(v).max()))
    a = np.abs(c['rgx'])
    assert 2.0 ** -3 <= a.max() <= 1.0, float(a.max())
    nz = a[a > 0]
    assert nz.size > 0.5 * a.size
    assert (nz < 2.0 ** -14).mean() <= 0.02, float((nz < 2.0 ** -14).mean())
    assert np.isfinite(c['rgw']).all()
    for m in split(c['rgw'], din, hid, nl):
        assert np.abs(m).max() > 0
    assert np.isfinite(c['floor_dx']) and all(np.isfinite(f) for f in c['floor_w'])


# ---- the bars (tests/test_gpu_ffmlp.py states them again where it uses them)
DX_TOL = 4e-3          # |got - ref| <= DX_TOL (|ref| + max |ref|), every element
W_L2, W_MAX = 2e-3, 3e-3


def dx_errors(got, ref):
    """(worst element error in units of the bar's right-hand side / DX_TOL, i.e. |got-ref| / (|ref| + max|ref|); max error / max)"""
    d = np.abs(got - ref)
    return float((d / (np.abs(ref) + np.abs(ref).max())).max()), float(d.max() / np.abs(ref).max())


def w_errors(got, ref, din, hid, nl):
    """per weight-gradient matrix: (relative L2, max error / max)"""
    return [(float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max()))
            for a, b in zip(split(got, din, hid, nl), split(ref, din, hid, nl))]
