"""GPU parity: MFMA fused MLP vs the numpy oracle and the reference-derived golden vectors."""
import os

import numpy as np
import pytest
import torch

import oracle
from network_cases import close_except_relu_flips as _close_except_relu_flips   # (shared with test_gpu_network_kernels.py)

pytestmark = pytest.mark.gpu


def cu16(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda().half()   # (a copy: the shared reference arrays are read-only)


def _be():
    from ffmlp.backend import _backend
    return _backend


def _run_forward(x, w, din, hid, nl, act=0, out_act=6, train=True):
    B = x.shape[0]
    xt, wt = cu16(x), cu16(w)
    out = torch.empty(B, 16, device='cuda', dtype=torch.half)
    if train:
        fb = torch.empty(nl, B, hid, device='cuda', dtype=torch.half)
        _be().ffmlp_forward(xt, wt, B, din, 16, hid, nl, act, out_act, fb, out)
        return out, fb, xt, wt
    buf = torch.empty(B, hid, device='cuda', dtype=torch.half)
    _be().ffmlp_inference(xt, wt, B, din, 16, hid, nl, act, out_act, buf, out)
    return out, None, xt, wt


CFGS = [(32, 64, 2), (32, 64, 3), (16, 64, 2), (64, 64, 2), (48, 64, 4), (32, 32, 2), (16, 32, 3), (64, 32, 4)]


@pytest.mark.parametrize('din,hid,nl', CFGS)
@pytest.mark.parametrize('B', [128, 1152, 16384])
def test_forward_inference_backward(din, hid, nl, B):
    rng = np.random.default_rng(din * 1000 + hid * 10 + nl)
    n_params = hid * (din + hid * (nl - 1) + 16)
    w = oracle.round_fp16(rng.uniform(-1, 1, n_params) * np.sqrt(3 / hid))
    x = oracle.round_fp16(rng.uniform(-1, 1, (B, din)))
    out, fb, xt, wt = _run_forward(x, w, din, hid, nl)
    ref, rfb = oracle.ffmlp_forward(x, w, din, 16, hid, nl)
    got = out.float().cpu().numpy()
    # fp16 outputs, fp32 accumulation: 1e-3 relative (BASELINE.json) with an absolute floor of one fp16 ulp at the output scale
    scale = np.abs(ref).max()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3 * scale)
    out_i, _, _, _ = _run_forward(x, w, din, hid, nl, train=False)
    assert torch.equal(out_i, out)
    # backward
    g = oracle.round_fp16(rng.normal(size=(B, 16)) * 0.1)
    gt = cu16(g)
    gi = torch.zeros(B, din, device='cuda', dtype=torch.half)
    gw = torch.zeros(n_params, device='cuda', dtype=torch.half)
    bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
    _be().ffmlp_backward(gt, xt, wt, fb, B, din, 16, hid, nl, 0, 6, True, bb, gi, gw)
    rgx, rgw = oracle.ffmlp_backward(g, x, w, rfb, din, 16, hid, nl)
    gx = gi.float().cpu().numpy()
    _close_except_relu_flips(gx, rgx, 4e-3, bulk=0.995 if nl <= 4 else 0.98)  # every extra ReLU layer adds mask flips
    gwn = gw.float().cpu().numpy()
    # weight gradients are sums over the batch: relative to the gradient scale of each matrix
    assert np.isfinite(gwn).all()
    # ReLU masks come from fp16 activations that the two sides sum in different orders: a unit whose pre-activation rounds to the other
    # side of zero flips one (sample, unit) entry of dZ.  The flip count grows with depth and width (measured on MI355X, tools/_dbg.py:
    # relative L2 2e-4 for 2-layer 64-wide nets, 1.6e-3 for 128 x 2, 5e-3 for 64 x 6, 8e-3 for 128 x 5) -- the bar scales with both
    flips = max(1, nl - 1) * (2 if hid >= 128 else 1)
    err = np.abs(gwn - rgw).max() / np.abs(rgw).max()
    assert err < 3e-3 * flips, err
    assert np.linalg.norm(gwn - rgw) / np.linalg.norm(rgw) < 2e-3 * flips
    # without dL/dx the weight gradients are unchanged and grad_inputs is not touched
    gw2 = torch.zeros_like(gw)
    dummy = torch.zeros(1, device='cuda', dtype=torch.half)
    bb.zero_()
    _be().ffmlp_backward(gt, xt, wt, fb, B, din, 16, hid, nl, 0, 6, False, bb, dummy, gw2)
    assert torch.equal(gw2, gw) and dummy.item() == 0


# every hidden width the reference accepts (ffmlp.py:112: 16, 32, 64, 128, 256), deeper stacks than the register-resident backward
# holds (> 4 hidden layers) and inputs wider than 64: the layered kernels
CFGS_LAYERED = [(32, 16, 2), (16, 16, 3), (32, 128, 2), (64, 128, 3), (32, 256, 2), (48, 256, 3), (32, 64, 6), (96, 64, 2), (32, 32, 8),
                (128, 128, 2), (32, 128, 5)]


@pytest.mark.parametrize('din,hid,nl', CFGS_LAYERED)
@pytest.mark.parametrize('B', [128, 4224])
def test_all_reference_shapes_forward_inference_backward(din, hid, nl, B):
    test_forward_inference_backward(din, hid, nl, B)


def test_layered_kernels_agree_with_register_resident_ones():
    """NGP_FF_LAYERED forces the matmul-by-matmul kernels on an instant-ngp shape: forward and dL/dx run the same MFMA sequence per output
    (bit-identical), the weight gradients differ only in the order the tiles are summed"""
    import _ngp_capi as capi
    rng = np.random.default_rng(5)
    for din, hid, nl in ((32, 64, 2), (32, 64, 3), (16, 32, 2)):
        B = 8192
        n_params = hid * (din + hid * (nl - 1) + 16)
        xt = cu16(rng.uniform(-1, 1, (B, din)))
        wt = cu16(rng.uniform(-1, 1, n_params) * np.sqrt(3 / hid))
        gt = cu16(rng.normal(size=(B, 16)) * 0.1)
        st = capi.stream()
        res = []
        for flags in (0, capi.NGP_FF_LAYERED):
            out = torch.empty(B, 16, device='cuda', dtype=torch.half)
            fb = torch.empty(nl, B, hid, device='cuda', dtype=torch.half)
            capi.check(capi.lib.ngp_ffmlp_forward_ex(xt.data_ptr(), wt.data_ptr(), B, din, 16, hid, nl, 0, 6, fb.data_ptr(), out.data_ptr(), flags, st))
            out_i = torch.empty(B, 16, device='cuda', dtype=torch.half)
            scratch = torch.empty(B, hid, device='cuda', dtype=torch.half)
            capi.check(capi.lib.ngp_ffmlp_inference_ex(xt.data_ptr(), wt.data_ptr(), B, din, 16, hid, nl, 0, 6, scratch.data_ptr(), out_i.data_ptr(),
                                                       flags, st))
            assert torch.equal(out, out_i)
            gi = torch.zeros(B, din, device='cuda', dtype=torch.half)
            gw = torch.zeros(n_params, device='cuda', dtype=torch.half)
            bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
            nbytes = 64 * n_params * 4
            ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
            capi.check(capi.lib.ngp_ffmlp_backward_ws(gt.data_ptr(), xt.data_ptr(), wt.data_ptr(), fb.data_ptr(), B, din, 16, hid, nl, 0, 6, 1,
                                                      bb.data_ptr(), gi.data_ptr(), gw.data_ptr(), flags, ws.data_ptr(), nbytes, st))
            gw_nows = torch.zeros_like(gw)
            if flags:  # without a workspace: one chunk, direct store -- same sums up to fp32 order
                capi.check(capi.lib.ngp_ffmlp_backward_ws(gt.data_ptr(), xt.data_ptr(), wt.data_ptr(), fb.data_ptr(), B, din, 16, hid, nl, 0, 6, 1,
                                                          bb.data_ptr(), gi.data_ptr(), gw_nows.data_ptr(), flags, None, 0, st))
            res.append((out.clone(), fb.clone(), gi.clone(), gw.float().cpu().numpy(), gw_nows.float().cpu().numpy()))
        a, b = res
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        scale = np.abs(a[3]).max()
        assert np.abs(a[3] - b[3]).max() <= 2e-3 * scale and np.abs(b[4] - b[3]).max() <= 2e-3 * scale


@pytest.mark.parametrize('din,hid,nl', [(64, 64, 4), (32, 64, 3)])
def test_backward_many_tiles_per_wave(din, hid, nl):
    """2^17 samples = 4096 tiles of 32 on ~1024 resident waves: every wave walks several tiles, so the operand prefetch is exercised
    in both of its forms (two stage buffers per wave; a single one when the 64-input 4-layer weight image leaves no room for two)."""
    B = 1 << 17
    rng = np.random.default_rng(77 + din + nl)
    n_params = hid * (din + hid * (nl - 1) + 16)
    w = oracle.round_fp16(rng.uniform(-1, 1, n_params) * np.sqrt(3 / hid))
    x = oracle.round_fp16(rng.uniform(-1, 1, (B, din)))
    out, fb, xt, wt = _run_forward(x, w, din, hid, nl)
    ref, rfb = oracle.ffmlp_forward(x, w, din, 16, hid, nl)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())
    g = oracle.round_fp16(rng.normal(size=(B, 16)) * 0.1)
    gi = torch.zeros(B, din, device='cuda', dtype=torch.half)
    gw = torch.zeros(n_params, device='cuda', dtype=torch.half)
    bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
    _be().ffmlp_backward(cu16(g), xt, wt, fb, B, din, 16, hid, nl, 0, 6, True, bb, gi, gw)
    rgx, rgw = oracle.ffmlp_backward(g, x, w, rfb, din, 16, hid, nl)
    _close_except_relu_flips(gi.float().cpu().numpy(), rgx, 4e-3)
    gwn = gw.float().cpu().numpy()
    assert np.isfinite(gwn).all()
    assert np.linalg.norm(gwn - rgw) / np.linalg.norm(rgw) < 2e-3


def test_backward_is_deterministic():
    rng = np.random.default_rng(0)
    din, hid, nl, B = 32, 64, 2, 1 << 17
    n_params = hid * (din + hid * (nl - 1) + 16)
    w = oracle.round_fp16(rng.uniform(-1, 1, n_params) * np.sqrt(3 / hid))
    x = oracle.round_fp16(rng.uniform(-1, 1, (B, din)))
    out, fb, xt, wt = _run_forward(x, w, din, hid, nl)
    gt = cu16(rng.normal(size=(B, 16)) * 0.01)
    res = []
    for _ in range(3):
        gi = torch.zeros(B, din, device='cuda', dtype=torch.half)
        gw = torch.zeros(n_params, device='cuda', dtype=torch.half)
        bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
        _be().ffmlp_backward(gt, xt, wt, fb, B, din, 16, hid, nl, 0, 6, True, bb, gi, gw)
        res.append((gi.clone(), gw.clone()))
    assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])


def test_transposition_is_detected():
    # asymmetric weights / one-hot inputs: output column j of sample n must be exactly W_out[j,:] . relu(W_in[:,k]) etc.
    din, hid, nl, B = 32, 64, 2, 128
    n_params = hid * (din + hid * (nl - 1) + 16)
    w = np.zeros(n_params, np.float32)
    Win = w[:hid * din].reshape(hid, din); Wh = w[hid * din:hid * din + hid * hid].reshape(hid, hid); Wo = w[hid * din + hid * hid:].reshape(16, hid)
    for k in range(din):
        Win[(3 * k + 1) % hid, k] = 1.0          # input k feeds hidden unit (3k+1)%64
    for i in range(hid):
        Wh[(5 * i + 2) % hid, i] = 1.0 + i / 64   # permutation with distinct gains
    for j in range(16):
        Wo[j, (7 * j + 3) % hid] = 0.5 + j / 16
    x = np.zeros((B, din), np.float32)
    for n in range(B):
        x[n, n % din] = 1.0 + (n // din)
    out, fb, _, _ = _run_forward(x, w, din, hid, nl)
    ref, _ = oracle.ffmlp_forward(oracle.round_fp16(x), oracle.round_fp16(w), din, 16, hid, nl)
    assert np.array_equal(out.float().cpu().numpy(), ref.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize('act', [1, 2, 3, 4, 5, 6])
def test_other_activations_forward(act):
    rng = np.random.default_rng(act)
    din, hid, nl, B = 32, 64, 2, 512
    n_params = hid * (din + hid * (nl - 1) + 16)
    w = oracle.round_fp16(rng.uniform(-1, 1, n_params) * 0.1)
    x = oracle.round_fp16(rng.uniform(-1, 1, (B, din)))
    out, fb, _, _ = _run_forward(x, w, din, hid, nl, act=act, out_act=3 if act == 6 else 6)
    ref, _ = oracle.ffmlp_forward(x, w, din, 16, hid, nl, activation=act, output_activation=3 if act == 6 else 6)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=3e-3, atol=3e-3)


def test_against_reference_mlp_golden(golden_dir):
    # golden outputs/gradients of the reference's own nn.Linear stack (testing/test_ffmlp.py:11-43), fp16-representable data
    from ffmlp import FFMLP
    z = np.load(os.path.join(golden_dir, 'mlp_ref.npz'))
    for name in ('sigma', 'color', 'test', 'narrow'):
        din, dout, hid, nl = [int(v) for v in z[name + '_cfg']]
        net = FFMLP(din, dout, hid, nl).cuda()
        with torch.no_grad():
            net.weights.copy_(torch.from_numpy(z[name + '_w']).float())
        x = torch.from_numpy(z[name + '_x']).float().cuda().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.float16):
            y = net(x)
        assert y.dtype == torch.float16 and y.shape == (x.shape[0], dout)
        ref = z[name + '_y']
        np.testing.assert_allclose(y.float().detach().cpu().numpy(), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).max())
        y.backward(torch.from_numpy(z[name + '_gy']).cuda().half())
        gx, gw = z[name + '_gx'], z[name + '_gw']
        _close_except_relu_flips(x.grad.cpu().numpy(), gx, 6e-3)
        got_w = net.weights.grad.float().cpu().numpy()
        # the float64 golden gradients see no fp16 activation rounding: one ReLU unit sitting at a pre-activation of ~1e-5
        # can flip (tools/dbg1.py found exactly one such row in 'color' and 'test'), which moves single weight-gradient
        # entries by a few percent of the largest entry; the tight check is the one against the fp16-rounding oracle below
        assert np.linalg.norm(got_w - gw) / np.linalg.norm(gw) < 3e-2
        _, fb = oracle.ffmlp_forward(z[name + '_x'], z[name + '_w'], din, 16, hid, nl)
        gy16 = np.zeros((x.shape[0], 16)); gy16[:, :dout] = oracle.round_fp16(z[name + '_gy'])
        _, gwo = oracle.ffmlp_backward(gy16, z[name + '_x'], z[name + '_w'], fb, din, 16, hid, nl)
        assert np.abs(got_w - gwo).max() / np.abs(gwo).max() < 3e-3
        # inference mode takes the other kernel and must agree
        net.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
            y2 = net(x)
        assert torch.equal(y2, y.detach())


def test_module_init_matches_reference_recipe():
    from ffmlp import FFMLP
    torch.manual_seed(123)
    net = FFMLP(32, 3, 64, 3)
    assert net.weights.shape == (11264,) and net.padded_output_dim == 16
    torch.manual_seed(42)
    ref = torch.empty(11264).uniform_(-(3 / 64) ** 0.5, (3 / 64) ** 0.5)
    assert torch.equal(net.weights.detach(), ref)


def test_bad_shapes_raise():
    be = _be()
    h = lambda *s: torch.zeros(*s, device='cuda', dtype=torch.half)
    with pytest.raises(RuntimeError, match='hidden_dim'):
        be.ffmlp_forward(h(128, 32), h(100000), 128, 32, 16, 48, 2, 0, 6, h(2, 128, 48), h(128, 16))
    with pytest.raises(RuntimeError, match='LDS'):  # the only shapes refused: a single layer larger than the LDS of a CU
        be.ffmlp_forward(h(128, 512), h(256 * (512 + 256 + 16)), 128, 512, 16, 256, 2, 0, 6, h(2, 128, 256), h(128, 16))
    with pytest.raises(RuntimeError, match='Half'):
        be.ffmlp_forward(torch.zeros(128, 32, device='cuda'), h(7168), 128, 32, 16, 64, 2, 0, 6, h(2, 128, 64), h(128, 16))
    with pytest.raises(RuntimeError, match='128'):
        be.ffmlp_forward(h(100, 32), h(7168), 100, 32, 16, 64, 2, 0, 6, h(2, 100, 64), h(100, 16))


def test_empty_batch_backward_returns_zero_weight_gradient():
    """the wrappers hand ffmlp_backward uninitialised grad_weights (every kernel overwrites them); with B == 0 no kernel runs, so
    the C entry must write the zeros itself -- also through nerf/network.py's fused Linear stacks under an all-False mask"""
    from ffmlp import FFMLP
    from ffmlp.ffmlp import ffmlp_forward
    torch.manual_seed(0)
    net = FFMLP(32, 16, 64, 2).cuda()
    x = torch.zeros(0, 32, device='cuda', dtype=torch.half, requires_grad=True)
    for _ in range(3):   # (fresh uninitialised buffers every time: garbage would show up sooner or later)
        torch.empty(net.weights.numel(), device='cuda', dtype=torch.half).fill_(7.0)
        with torch.autocast('cuda', dtype=torch.float16):   # (the wrappers cast under autocast, as the reference's custom_fwd does)
            out = ffmlp_forward(x, net.weights, 32, 16, 64, 2, 0, 6, False, True)
        assert out.shape == (0, 16)
        gw, = torch.autograd.grad(out.float().sum(), net.weights, allow_unused=True)
        assert gw is not None and float(gw.abs().max()) == 0.0
    from nerf.network import NeRFNetwork
    m = NeRFNetwork(bound=1, cuda_ray=False).cuda()
    d = torch.nn.functional.normalize(torch.randn(8, 3, device='cuda'), dim=-1)
    geo = torch.randn(8, 15, device='cuda', requires_grad=True)
    with torch.autocast('cuda', dtype=torch.float16):
        rgb = m.color(torch.zeros(8, 3, device='cuda'), d, mask=torch.zeros(8, dtype=torch.bool, device='cuda'), geo_feat=geo)
    assert float(rgb.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# Every activation (0 ReLU, 1 Exp, 2 Sine, 3 Sigmoid, 4 Squareplus, 5 Softplus, 6 None) through forward, inference and backward.
# Cases, data and reference values: tests/ffmlp_act_cases.py (the same table tests/test_ffmlp_activations.py checks on the CPU).
#
# Which test launches which kernel with activation != 0, each at B = 128 (4 tiles, one workgroup, direct weight-gradient store) and
# B = 4224 (132 tiles, 33 workgroups, fp32 slabs + k_ffmlp_reduce_slabs; several chunks in the layered path with a workspace):
#   test_activation_backward_register_resident   k_ffmlp_backward_paired<W, J, 1|2, false> and k_ffmlp_backward<W, J, 3, false>,
#                                                W in {32, 64}, J in {1, 2} (the comment column of FAST_SHAPES names each)
#   test_activation_backward_single_wave         k_ffmlp_backward<64,1,1,*>, <64,2,2,*>, <32,1,2,*>, <32,2,1,*> (NGP_FF_SINGLE_WAVE)
#   test_activation_backward_layered             k_ffmlp_dgrad_layered<16|32|64|128|256, false>, k_ffmlp_wgrad, k_ffmlp_reduce_slabs
#   test_activation_forward_and_inference        k_ffmlp_forward<16|32|64, *, false>, k_ffmlp_forward_wide<128, *, false>,
#                                                k_ffmlp_forward_layered<256|64, *> (256-wide, 6 layers, 96 inputs, NGP_FF_LAYERED)
#
# Bars.  There are no ReLU mask flips for activations 1-6, so EVERY element is held to the bar:
#   dL/dx          |got - ref| <= 4e-3 (|ref| + max |ref|)
#   dL/dW          per matrix: relative L2 < 2e-3 and max error < 3e-3 of the maximum
#   forward        rtol = atol / max |ref| = 3e-3 (__expf / __sinf / __logf), 1e-3 with ReLU hidden layers and no output activation
# The reference's own noise is measured per case (ffmlp_act_cases.backward_case: the float32 oracle against the float64 one at the
# same rounding points, 1e-4 .. 5e-4 of max |dx| -- one flipped fp16 rounding); a case whose 4 x floor exceeds a bar is held to
# 4 x its floor instead.  On the table as it stands no case needs that (EXPERIMENTS.md, "FFMLP activations parity").
# ------------------------------------------------------------------------------------------------------------------------------
import ffmlp_act_cases as C


def _capi():
    import _ngp_capi as capi
    return capi


def _forward_capi(xt, wt, B, din, hid, nl, act, out_act, flags, train=True):
    capi = _capi()
    out = torch.empty(B, 16, device='cuda', dtype=torch.half)
    if train:
        fb = torch.empty(nl, B, hid, device='cuda', dtype=torch.half)
        capi.check(capi.lib.ngp_ffmlp_forward_ex(xt.data_ptr(), wt.data_ptr(), B, din, 16, hid, nl, act, out_act, fb.data_ptr(), out.data_ptr(), flags,
                                                 capi.stream()))
        return out, fb
    scratch = torch.empty(B, hid, device='cuda', dtype=torch.half)
    capi.check(capi.lib.ngp_ffmlp_inference_ex(xt.data_ptr(), wt.data_ptr(), B, din, 16, hid, nl, act, out_act, scratch.data_ptr(), out.data_ptr(), flags,
                                               capi.stream()))
    return out, None


def _backward_capi(gt, xt, wt, fb, B, din, hid, nl, act, out_act=6, flags=0, workspace=False, with_dx=True):
    """-> (grad_inputs fp16 tensor, grad_weights fp16 tensor); the outputs start as NaN so that anything left unwritten shows"""
    capi = _capi()
    gi = torch.full((B, din), float('nan'), device='cuda', dtype=torch.half)
    gw = torch.full((C.n_params(din, hid, nl),), float('nan'), device='cuda', dtype=torch.half)
    bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
    ws, nbytes = None, 0
    if workspace:
        nbytes = capi.lib.ngp_ffmlp_backward_workspace_bytes(B, din, hid, nl)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    capi.check(capi.lib.ngp_ffmlp_backward_ws(gt.data_ptr(), xt.data_ptr(), wt.data_ptr(), fb.data_ptr(), B, din, 16, hid, nl, act, out_act,
                                              1 if with_dx else 0, bb.data_ptr(), gi.data_ptr(), gw.data_ptr(), flags,
                                              ws.data_ptr() if ws is not None else None, nbytes, capi.stream()))
    torch.cuda.synchronize()
    return gi, gw


def _forward_bar(act, out_act):
    return 1e-3 if act == 0 and out_act == 6 else 3e-3


def _check_forward(out, ref, act, out_act, label):
    got = out.float().cpu().numpy()
    tol = _forward_bar(act, out_act)
    scale = np.abs(ref).max()
    err = np.abs(got - ref) / (np.abs(ref) + scale)
    print(f'PARITY fwd {label}: max |err| / (|ref| + max) {err.max():.2e} (bar {tol:.0e})')
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * scale)


def _check_backward(gi, gw, c, din, hid, nl, act, label):
    """dL/dx and every weight-gradient matrix against the oracle values of case c, every element (activations 1-6), or with the ReLU
    mask-flip allowance of test_forward_inference_backward (activation 0)"""
    gx, gwn = gi.float().cpu().numpy(), gw.float().cpu().numpy()
    assert np.isfinite(gx).all() and np.isfinite(gwn).all(), label
    rgx, rgw = c['rgx'], c['rgw']
    e_el, e_max = C.dx_errors(gx, rgx)
    werr = C.w_errors(gwn, rgw, din, hid, nl)
    print(f'PARITY bwd {label}: dx elem {e_el:.2e} max {e_max:.2e} floor {c["floor_dx"]:.1e} | dW L2 {max(w[0] for w in werr):.2e} '
          f'max {max(w[1] for w in werr):.2e} floor {max(c["floor_w"]):.1e}')
    if act == 0:
        _close_except_relu_flips(gx, rgx, C.DX_TOL)
        flips = max(1, nl - 1)
        for l2, mx in werr:
            assert mx < C.W_MAX * flips and l2 < C.W_L2 * flips, (label, werr)
        return
    amax = np.abs(rgx).max()
    # a case may exceed the project bar only where 4 x the oracle's own float32-vs-float64 noise explains it
    bound = np.maximum(C.DX_TOL * (np.abs(rgx) + amax), 4 * c['floor_dx'] * amax)
    bad = np.abs(gx - rgx) > bound
    assert not bad.any(), (label, int(bad.sum()), e_el, e_max)
    for (l2, mx), fl in zip(werr, c['floor_w']):
        assert l2 < max(C.W_L2, 4 * fl) and mx < max(C.W_MAX, 4 * fl), (label, werr)


def _id(v):
    return '-'.join(str(x) for x in v)


@pytest.mark.parametrize('case', C.FAST_CASES, ids=_id)
@pytest.mark.parametrize('B', C.BATCHES)
def test_activation_backward_register_resident(case, B):
    din, hid, nl, act = case
    c = C.backward_case(din, hid, nl, act, B)
    C.check_conditions(c, din, hid, nl)
    label = f'fast {din}->{hid}x{nl} {C.ACT_NAMES[act]} B={B}'
    out, fb, xt, wt = _run_forward(c['x'], c['w'], din, hid, nl, act=act)
    _check_forward(out, c['ref'], act, 6, label)
    gt = cu16(c['g'])
    n_params = C.n_params(din, hid, nl)
    gi = torch.full((B, din), float('nan'), device='cuda', dtype=torch.half)
    gw = torch.full((n_params,), float('nan'), device='cuda', dtype=torch.half)
    bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
    _be().ffmlp_backward(gt, xt, wt, fb, B, din, 16, hid, nl, act, 6, True, bb, gi, gw)
    _check_backward(gi, gw, c, din, hid, nl, act, label)
    # without dL/dx the weight gradients are unchanged and grad_inputs is not touched
    gw2 = torch.full_like(gw, float('nan'))
    dummy = torch.zeros(1, device='cuda', dtype=torch.half)
    bb.zero_()
    _be().ffmlp_backward(gt, xt, wt, fb, B, din, 16, hid, nl, act, 6, False, bb, dummy, gw2)
    assert torch.equal(gw2, gw) and dummy.item() == 0


@pytest.mark.parametrize('case', C.SINGLE_WAVE_CASES, ids=_id)
@pytest.mark.parametrize('B', C.BATCHES)
def test_activation_backward_single_wave(case, B):
    """NGP_FF_SINGLE_WAVE runs k_ffmlp_backward<W, J, 1|2, *> where the paired kernel would: role 1 of the paired kernel walks the same dgrad
    chain with the same MFMA sequence per output, so dL/dx is bit-identical; the weight gradients differ in fp32 summation order only."""
    din, hid, nl, act = case
    capi = _capi()
    c = C.backward_case(din, hid, nl, act, B)
    C.check_conditions(c, din, hid, nl)
    label = f'single-wave {din}->{hid}x{nl} {C.ACT_NAMES[act]} B={B}'
    xt, wt, gt = cu16(c['x']), cu16(c['w']), cu16(c['g'])
    out, fb = _forward_capi(xt, wt, B, din, hid, nl, act, 6, 0)
    gi_p, gw_p = _backward_capi(gt, xt, wt, fb, B, din, hid, nl, act)
    gi_s, gw_s = _backward_capi(gt, xt, wt, fb, B, din, hid, nl, act, flags=capi.NGP_FF_SINGLE_WAVE)
    _check_backward(gi_s, gw_s, c, din, hid, nl, act, label)
    assert torch.equal(gi_s, gi_p)
    a, b = gw_s.float().cpu().numpy(), gw_p.float().cpu().numpy()
    assert np.abs(a - b).max() <= 2e-3 * np.abs(b).max()


@pytest.mark.parametrize('case', C.LAYERED_CASES, ids=_id)
@pytest.mark.parametrize('B', C.BATCHES)
def test_activation_backward_layered(case, B):
    """once with the workspace ngp_ffmlp_backward_workspace_bytes asks for (sample chunks + k_ffmlp_reduce_slabs where B allows more than
    one chunk) and once with NULL (one chunk, direct store): both against the oracle, and against each other to fp32 summation order"""
    din, hid, nl, act, forced = case
    capi = _capi()
    flags = capi.NGP_FF_LAYERED if forced else 0
    c = C.backward_case(din, hid, nl, act, B)
    C.check_conditions(c, din, hid, nl)
    label = f'layered{"(forced)" if forced else ""} {din}->{hid}x{nl} {C.ACT_NAMES[act]} B={B}'
    xt, wt, gt = cu16(c['x']), cu16(c['w']), cu16(c['g'])
    out, fb = _forward_capi(xt, wt, B, din, hid, nl, act, 6, flags)
    _check_forward(out, c['ref'], act, 6, label)
    n_params = C.n_params(din, hid, nl)
    res = []
    for with_ws in (True, False):
        if forced:   # (the workspace query answers 0 for a shape the register-resident kernels serve: size it as the layered path does)
            gi = torch.full((B, din), float('nan'), device='cuda', dtype=torch.half)
            gw = torch.full((n_params,), float('nan'), device='cuda', dtype=torch.half)
            bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
            nbytes = 64 * n_params * 4 if with_ws else 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda') if with_ws else None
            capi.check(capi.lib.ngp_ffmlp_backward_ws(gt.data_ptr(), xt.data_ptr(), wt.data_ptr(), fb.data_ptr(), B, din, 16, hid, nl, act, 6, 1,
                                                      bb.data_ptr(), gi.data_ptr(), gw.data_ptr(), flags, ws.data_ptr() if with_ws else None, nbytes,
                                                      capi.stream()))
            torch.cuda.synchronize()
        else:
            gi, gw = _backward_capi(gt, xt, wt, fb, B, din, hid, nl, act, flags=flags, workspace=with_ws)
        _check_backward(gi, gw, c, din, hid, nl, act, label + (' ws' if with_ws else ' no-ws'))
        res.append((gi, gw.float().cpu().numpy()))
    assert torch.equal(res[0][0], res[1][0])
    assert np.abs(res[0][1] - res[1][1]).max() <= 2e-3 * np.abs(res[1][1]).max()
    if forced:   # the register-resident kernels run the same MFMA sequence per output: dL/dx bit for bit, dW to fp32 summation order
        out_r, fb_r = _forward_capi(xt, wt, B, din, hid, nl, act, 6, 0)
        assert torch.equal(out_r, out) and torch.equal(fb_r, fb)
        gi_r, gw_r = _backward_capi(gt, xt, wt, fb_r, B, din, hid, nl, act)
        assert torch.equal(gi_r, res[0][0])
        assert np.abs(gw_r.float().cpu().numpy() - res[1][1]).max() <= 2e-3 * np.abs(res[1][1]).max()


@pytest.mark.parametrize('case', C.OUT_ACT_IGNORED_CASES, ids=_id)
def test_backward_ignores_output_activation(case):
    """the backward takes grad as dL/d(what the output layer's matmul produced): output_activation is a forward-only argument, as in the
    reference (ffmlp.cu:780)"""
    din, hid, nl, act, _ = case
    B = 128
    c = C.backward_case(din, hid, nl, act, B)
    C.check_conditions(c, din, hid, nl)
    xt, wt, gt = cu16(c['x']), cu16(c['w']), cu16(c['g'])
    out, fb = _forward_capi(xt, wt, B, din, hid, nl, act, 6, 0)
    res = [_backward_capi(gt, xt, wt, fb, B, din, hid, nl, act, out_act=oa) for oa in (0, 3, 6)]
    _check_backward(res[2][0], res[2][1], c, din, hid, nl, act, f'out_act {din}->{hid}x{nl} {C.ACT_NAMES[act]}')
    for gi, gw in res[:2]:
        assert torch.equal(gi, res[2][0]) and torch.equal(gw, res[2][1])


@pytest.mark.parametrize('case', C.FORWARD_CASES, ids=_id)
@pytest.mark.parametrize('B', C.BATCHES)
def test_activation_forward_and_inference(case, B):
    """training forward against the oracle, inference bit-identical with it, and -- where the register-resident kernel serves the shape --
    the layered kernel (NGP_FF_LAYERED) bit-identical with the register-resident one"""
    din, hid, nl, act, out_act, forced = case
    capi = _capi()
    c = C.forward_case(din, hid, nl, act, out_act, B)
    C.check_forward_conditions(c)
    label = f'{din}->{hid}x{nl} {C.ACT_NAMES[act]}/{C.ACT_NAMES[out_act]}{" layered(forced)" if forced else ""} B={B}'
    xt, wt = cu16(c['x']), cu16(c['w'])
    flags = capi.NGP_FF_LAYERED if forced else 0
    out, _ = _forward_capi(xt, wt, B, din, hid, nl, act, out_act, flags)
    _check_forward(out, c['ref'], act, out_act, label)
    out_i, _ = _forward_capi(xt, wt, B, din, hid, nl, act, out_act, flags, train=False)
    assert torch.equal(out_i, out)
    if forced:
        out_r, _ = _forward_capi(xt, wt, B, din, hid, nl, act, out_act, 0)
        out_ri, _ = _forward_capi(xt, wt, B, din, hid, nl, act, out_act, 0, train=False)
        assert torch.equal(out_r, out) and torch.equal(out_ri, out)
    # the pybind entry points take the same route
    out_p, _, _, _ = _run_forward(c['x'], c['w'], din, hid, nl, act=act, out_act=out_act)
    if not forced:
        assert torch.equal(out_p, out)


def test_module_with_sigmoid_activation():
    """FFMLP(32, 3, 64, 3, activation='sigmoid') under autocast: y, x.grad and weights.grad against the oracle; eval() takes the inference
    kernel and must agree bit for bit"""
    from ffmlp import FFMLP
    din, hid, nl, act = C.MODULE_CASE
    B, dout = C.MODULE_B, C.MODULE_OUT
    c = C.backward_case(din, hid, nl, act, B, dout)
    C.check_conditions(c, din, hid, nl)
    net = FFMLP(din, dout, hid, nl, activation='sigmoid').cuda()
    assert net.activation == 3 and net.weights.numel() == c['w'].size
    with torch.no_grad():
        net.weights.copy_(torch.tensor(c['w']))
    x = torch.tensor(c['x']).cuda().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = net(x)
    assert y.dtype == torch.float16 and y.shape == (B, dout)
    _check_forward(y.detach(), c['ref'][:, :dout], act, 6, 'module sigmoid')
    # the kernels see the padded 16-column output gradient: columns dout..15 of the case's g are zero
    y.backward(cu16(c['g'][:, :dout]))
    _check_backward(x.grad, net.weights.grad, c, din, hid, nl, act, 'module sigmoid')
    net.eval()
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        y2 = net(x)
    assert torch.equal(y2, y.detach())
