"""The oracle's activation-aware FFMLP backward, and the input conditions of every case the GPU activation tests use.  CPU only.

oracle.ffmlp_backward(activation=a) restates the reference's warp_activation_backward: the derivative factor is a function of the
STORED post-activation.  Finite differences of the forward pin that formula set; Sine is pinned as the pass-through it is."""
import numpy as np
import pytest

import oracle

import ffmlp_act_cases as C

DIN, HID, NL, B = 16, 16, 3, 4


def _fd_net(act):
    rng = np.random.default_rng(100 + act)
    w = rng.uniform(-1, 1, C.n_params(DIN, HID, NL)) * np.sqrt(3 / HID) * C.weight_scale(act)
    x = rng.uniform(-1, 1, (B, DIN))
    g = rng.normal(size=(B, 16))
    return x, w, g


def _loss(x, w, g, act):
    y, _ = oracle.ffmlp_forward(x, w, DIN, 16, HID, NL, activation=act, round_hidden=False, dtype=np.float64)
    return float((y * g).sum())


@pytest.mark.parametrize('act', [1, 3, 4, 5, 6])
def test_unrounded_backward_equals_finite_differences(act):
    """dL/dx (every entry) and dL/dW of the first and of a hidden matrix against central differences of the float64 forward, L = sum(y g).
    Bar 1e-5 of the gradient's maximum: the worst of these measures 1.5e-7 (sigmoid, eps 1e-6), the others ~3e-9."""
    x, w, g = _fd_net(act)
    _, fb = oracle.ffmlp_forward(x, w, DIN, 16, HID, NL, activation=act, round_hidden=False, dtype=np.float64)
    gx, gw = oracle.ffmlp_backward(g, x, w, fb, DIN, 16, HID, NL, round_hidden=False, activation=act)
    eps = 1e-6
    fd_x = np.zeros_like(x)
    for i in range(B):
        for j in range(DIN):
            xp, xm = x.copy(), x.copy()
            xp[i, j] += eps
            xm[i, j] -= eps
            fd_x[i, j] = (_loss(xp, w, g, act) - _loss(xm, w, g, act)) / (2 * eps)
    err = np.abs(gx - fd_x).max() / np.abs(fd_x).max()
    print(f'act {act}: dL/dx vs finite differences {err:.2e}')
    assert err < 1e-5, err
    # W_in [HID, DIN] and the first hidden matrix [HID, HID]
    n0, n1 = HID * DIN, HID * DIN + HID * HID
    fd_w = np.zeros(n1)
    for i in range(n1):
        wp, wm = w.copy(), w.copy()
        wp[i] += eps
        wm[i] -= eps
        fd_w[i] = (_loss(x, wp, g, act) - _loss(x, wm, g, act)) / (2 * eps)
    for lo, hi in ((0, n0), (n0, n1)):
        err = np.abs(gw[lo:hi] - fd_w[lo:hi]).max() / np.abs(fd_w[lo:hi]).max()
        print(f'act {act}: dL/dW[{lo}:{hi}] vs finite differences {err:.2e}')
        assert err < 1e-5, err


def test_sine_backward_is_the_none_backward_on_the_same_buffer():
    x, w, g = _fd_net(2)
    for rounded in (False, True):
        _, fb = oracle.ffmlp_forward(x, w, DIN, 16, HID, NL, activation=2, round_hidden=rounded, dtype=np.float64)
        a = oracle.ffmlp_backward(g, x, w, fb, DIN, 16, HID, NL, round_hidden=rounded, activation=2)
        b = oracle.ffmlp_backward(g, x, w, fb, DIN, 16, HID, NL, round_hidden=rounded, activation=6)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # and it is NOT the derivative of the sine forward
    _, fb = oracle.ffmlp_forward(x, w, DIN, 16, HID, NL, activation=2, round_hidden=False, dtype=np.float64)
    gx, _ = oracle.ffmlp_backward(g, x, w, fb, DIN, 16, HID, NL, round_hidden=False, activation=2)
    xp, xm = x.copy(), x.copy()
    xp[0, 0] += 1e-6
    xm[0, 0] -= 1e-6
    fd = (_loss(xp, w, g, 2) - _loss(xm, w, g, 2)) / 2e-6
    assert abs(gx[0, 0] - fd) > 1e-3 * abs(fd)


def test_default_backward_is_the_relu_backward():
    """activation=0 is the default and what every earlier caller gets: the mask y > 0"""
    rng = np.random.default_rng(3)
    din, hid, nl, b = 32, 64, 3, 128
    w = oracle.round_fp16(rng.uniform(-1, 1, C.n_params(din, hid, nl)) * np.sqrt(3 / hid))
    x = oracle.round_fp16(rng.uniform(-1, 1, (b, din)))
    g = oracle.round_fp16(rng.normal(size=(b, 16)) * 0.1)
    _, fb = oracle.ffmlp_forward(x, w, din, 16, hid, nl)
    a = oracle.ffmlp_backward(g, x, w, fb, din, 16, hid, nl)
    b_ = oracle.ffmlp_backward(g, x, w, fb, din, 16, hid, nl, activation=0)
    assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1])
    mats = oracle.ffmlp_split_weights(w, din, 16, hid, nl)
    gh = ((g.astype(np.float64) @ mats[3]) * (fb[2] > 0)).astype(np.float16).astype(np.float64)
    gh = ((gh @ mats[2]) * (fb[1] > 0)).astype(np.float16).astype(np.float64)
    gh = ((gh @ mats[1]) * (fb[0] > 0)).astype(np.float16).astype(np.float64)
    assert np.array_equal(a[0], gh @ mats[0])


@pytest.mark.parametrize('din,hid,nl,act', C.backward_case_table())
@pytest.mark.parametrize('B', C.BATCHES)
def test_backward_case_meets_the_input_conditions(din, hid, nl, act, B):
    c = C.backward_case(din, hid, nl, act, B)
    C.check_conditions(c, din, hid, nl)
    assert c['g'].shape == (B, 16) and np.array_equal(c['g'], oracle.round_fp16(c['g']))


def test_module_case_meets_the_input_conditions():
    din, hid, nl, act = C.MODULE_CASE
    c = C.backward_case(din, hid, nl, act, C.MODULE_B, C.MODULE_OUT)
    C.check_conditions(c, din, hid, nl)
    assert not c['g'][:, C.MODULE_OUT:].any() and c['g'][:, :C.MODULE_OUT].all(axis=0).any()


@pytest.mark.parametrize('case', C.FORWARD_CASES, ids=lambda c: '-'.join(str(v) for v in c))
@pytest.mark.parametrize('B', C.BATCHES)
def test_forward_case_meets_the_input_conditions(case, B):
    din, hid, nl, act, out_act, _ = case
    C.check_forward_conditions(C.forward_case(din, hid, nl, act, out_act, B))


def test_case_table_reaches_every_instantiation():
    """the twelve (W, IN_JB, NHM) instantiations of the register-resident backward, each with Softplus and None; all of 1-6 on the
    four named shapes; five layered widths; <64, 2, 2> under the single-wave flag"""
    inst = {(h, (d + 31) // 32, n - 1) for d, h, n in C.FAST_SHAPES}
    assert inst == {(w, j, m) for w in (32, 64) for j in (1, 2) for m in (1, 2, 3)}
    assert (64, 64, 4) in C.FAST_SHAPES and any(d % 32 for d, _, _ in C.FAST_SHAPES)
    for s in C.FAST_SHAPES:
        assert (*s, 5) in C.FAST_CASES and (*s, 6) in C.FAST_CASES
    for s in C.FAST_ALL_ACTS:
        assert all((*s, a) in C.FAST_CASES for a in C.SMOOTH)
    assert {h for _, h, _, a, _ in C.LAYERED_CASES if a != 0} == {16, 32, 64, 128, 256}
    assert all((32, 128, 2, a, 0) in C.LAYERED_CASES for a in C.SMOOTH)
    assert (64, 64, 3) in C.SINGLE_WAVE_SHAPES
    assert {h for _, h, _, a, _, _ in C.FORWARD_CASES if a != 0} == {16, 32, 64, 128, 256}
