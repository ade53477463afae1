"""The register-resident FFMLP backward kernels sum their waves' weight-gradient accumulators in one staged, parallel pass; the form they had
before -- one wave after the other into one LDS copy -- stays selectable as NGP_FF_SERIAL_FLUSH and is the reference here.  Both perform the
same fp32 additions in the same order, so every slab, every weight gradient and every input gradient must agree BIT FOR BIT (compared as
integers: the sign of a zero counts).  The inputs make the fp32 partial sums round (gradients of magnitude 2^10 against non-zero
activations), so a changed order of additions would show: test_the_partial_sums_of_these_inputs_round asserts that they do.

Batch sizes: 128 = one workgroup, direct fp16 store; 640 = five workgroups, one round of tiles; 32896 = 1028 tiles, workgroup 0 runs a second
round while the others do not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = [128, 640, 32896]


def _capi():
    import _ngp_capi as capi
    return capi


def _n_params(din, hid, nl):
    return hid * (din + hid * (nl - 1) + 16)


_inputs = {}


def _case(B, din, hid, nl, planar):
    """(x, w, dy, forward buffer) of a shape, made once: x row-major [B, din] or the encoder's planes [din/2, B, 2]"""
    key = (B, din, hid, nl, planar)
    if key not in _inputs:
        capi = _capi()
        g = torch.Generator(device='cuda').manual_seed(B + 7 * din + 11 * hid + 13 * nl)
        x = (torch.rand(B, din, device='cuda', generator=g) * 2 - 1).half()
        if planar:
            x = x.view(B, din // 2, 2).permute(1, 0, 2).contiguous()
        w = ((torch.rand(_n_params(din, hid, nl), device='cuda', generator=g) * 2 - 1) * (3 / hid) ** 0.5).half()
        dy = torch.randn(B, 16, device='cuda', generator=g).half() * 1024   # an exact scaling
        fb = torch.empty(nl, B, hid, device='cuda', dtype=torch.half)
        out = torch.empty(B, 16, device='cuda', dtype=torch.half)
        capi.check(capi.lib.ngp_ffmlp_forward_ex(x.data_ptr(), w.data_ptr(), B, din, 16, hid, nl, 0, 6, fb.data_ptr(), out.data_ptr(),
                                                 capi.NGP_FF_INPUT_PLANAR if planar else 0, capi.stream()))
        torch.cuda.synchronize()
        _inputs[key] = (x, w, dy, fb)
    return _inputs[key]


def _backward(B, din, hid, nl, flags, planar=False, with_dx=True, recompute=False):
    """-> (grad_inputs, grad_weights, backward_buffer); outputs start as NaN / zero so that anything left unwritten shows"""
    capi = _capi()
    x, w, dy, fb = _case(B, din, hid, nl, planar)
    if planar:
        flags |= capi.NGP_FF_INPUT_PLANAR | capi.NGP_FF_DX_PLANAR
    if recompute:
        flags |= capi.NGP_FF_RECOMPUTE
    gi = torch.full((B * din,), float('nan'), device='cuda', dtype=torch.half)
    gw = torch.full((_n_params(din, hid, nl),), float('nan'), device='cuda', dtype=torch.half)
    bb = torch.zeros(nl, B, hid, device='cuda', dtype=torch.half)
    capi.check(capi.lib.ngp_ffmlp_backward_ws(dy.data_ptr(), x.data_ptr(), w.data_ptr(), None if recompute else fb.data_ptr(), B, din, 16, hid, nl,
                                              0, 6, 1 if with_dx else 0, bb.data_ptr(), gi.data_ptr(), gw.data_ptr(), flags, None, 0,
                                              capi.stream()))
    torch.cuda.synchronize()
    return gi, gw, bb


def _slabs(bb, B, din, hid, nl):
    """the fp32 slabs a deferred backward left at the start of its backward_buffer, [n_slabs, n_params] (n_slabs = 0: stored directly)"""
    k = _capi().lib.ngp_ffmlp_backward_slab_count(B, din, hid, nl)
    n = _n_params(din, hid, nl)
    return bb.view(-1)[:2 * k * n].view(torch.float32).view(k, n)


def _same_bits(a, b, what):
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert torch.equal(a.contiguous().view(view), b.contiguous().view(view)), what


def _check_both_forms(B, din, hid, nl, flags=0, planar=False, with_dx=True, recompute=False, deferred=True):
    """the staged sum against the serial reference: deferred (the raw fp32 slabs) and reduced (grad_weights), and dL/dx"""
    capi = _capi()
    for defer in ((capi.NGP_FF_DEFER_REDUCE, 0) if deferred else (0,)):
        kw = dict(planar=planar, with_dx=with_dx, recompute=recompute)
        gi, gw, bb = _backward(B, din, hid, nl, flags | defer, **kw)
        gi_r, gw_r, bb_r = _backward(B, din, hid, nl, flags | defer | capi.NGP_FF_SERIAL_FLUSH, **kw)
        n_slabs = capi.lib.ngp_ffmlp_backward_slab_count(B, din, hid, nl) if defer else 0
        if n_slabs:
            s, s_r = _slabs(bb, B, din, hid, nl), _slabs(bb_r, B, din, hid, nl)
            assert torch.isfinite(s_r).all() and float(s_r.abs().max()) > 0
            _same_bits(s, s_r, 'slabs')
        else:   # reduced by the library, or stored directly by the one workgroup
            assert not torch.isnan(gw_r).any() and float(gw_r.float().abs().max()) > 0
            _same_bits(gw, gw_r, 'grad_weights')
        if with_dx:
            assert torch.isfinite(gi_r.float()).all() and float(gi_r.float().abs().max()) > 0
        _same_bits(gi, gi_r, 'grad_inputs')   # (without dL/dx: both untouched)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('planar', [False, True])
@pytest.mark.parametrize('with_dx', [True, False])
@pytest.mark.parametrize('nl', [2, 3])
def test_paired_kernel(nl, with_dx, planar, B):
    _check_both_forms(B, 32, 64, nl, planar=planar, with_dx=with_dx)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('nl', [2, 3])
def test_paired_kernel_that_recomputes_the_activations(nl, B):
    _check_both_forms(B, 32, 64, nl, recompute=True)
    _check_both_forms(B, 32, 64, nl, recompute=True, planar=True)


@pytest.mark.parametrize('B', BATCHES)
def test_paired_kernel_of_width_32(B):
    _check_both_forms(B, 32, 32, 3)
    _check_both_forms(B, 16, 32, 2, with_dx=False)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('nl', [2, 3, 4])
@pytest.mark.parametrize('hid', [64, 32])
def test_single_wave_kernel(hid, nl, B):
    """every wave holds every matrix.  (The 64-wide nets of 3 and 4 layers fill this kernel's register file and keep the serial form alone:
    both runs are then the same code, and agree trivially.)"""
    _check_both_forms(B, 32, hid, nl, flags=_capi().NGP_FF_SINGLE_WAVE, deferred=False)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('recompute', [False, True])
@pytest.mark.parametrize('nl', [2, 3])
def test_colour_entry_with_its_mid_epilogue(nl, recompute, B):
    capi = _capi()
    x, w, dy, fb = _case(B, 32, 64, nl, False)
    g = torch.Generator(device='cuda').manual_seed(B + nl)
    h16 = torch.randn(B, 16, device='cuda', generator=g).half()
    g_sigma = torch.randn(B, device='cuda', generator=g) * 0.01
    for defer in (capi.NGP_FF_DEFER_REDUCE, 0):
        res = []
        for serial in (0, capi.NGP_FF_SERIAL_FLUSH):
            g_h16 = torch.full((B, 16), float('nan'), device='cuda', dtype=torch.half)
            gw = torch.full_like(w, float('nan'))
            bb = torch.zeros(nl, B, 64, device='cuda', dtype=torch.half)
            flags = defer | serial | (capi.NGP_FF_RECOMPUTE if recompute else 0)
            capi.check(capi.lib.ngp_network_backward_color(dy.data_ptr(), x.data_ptr(), w.data_ptr(), None if recompute else fb.data_ptr(), B, nl,
                                                           bb.data_ptr(), g_sigma.data_ptr(), h16.data_ptr(), 1.3, g_h16.data_ptr(), gw.data_ptr(),
                                                           flags, capi.stream()))
            torch.cuda.synchronize()
            res.append((g_h16, gw, bb))
        (g_h16, gw, bb), (g_h16_r, gw_r, bb_r) = res
        assert torch.isfinite(g_h16_r.float()).all() and float(g_h16_r.float().abs().max()) > 0
        _same_bits(g_h16, g_h16_r, 'grad_h16')
        if defer and capi.lib.ngp_ffmlp_backward_slab_count(B, 32, 64, nl):
            s_r = _slabs(bb_r, B, 32, 64, nl)
            assert torch.isfinite(s_r).all() and float(s_r.abs().max()) > 0
            _same_bits(_slabs(bb, B, 32, 64, nl), s_r, 'slabs')
        else:
            assert not torch.isnan(gw_r).any() and float(gw_r.float().abs().max()) > 0
            _same_bits(gw, gw_r, 'grad_w_color')


@pytest.mark.parametrize('B', [640, 32896])
def test_the_partial_sums_of_these_inputs_round(B):
    """The output layer's block of every slab against its float64 sum over the workgroup's samples: close (the decomposition is right), and
    not equal -- the fp32 sums round, so an order of additions other than the reference's would change bits.  The hidden activations are
    read through the public inference entry: an output layer of unit rows copies sixteen of them exactly."""
    capi = _capi()
    din, hid, nl = 32, 64, 2
    x, w, dy, fb = _case(B, din, hid, nl, False)
    act = torch.empty(B, hid, device='cuda', dtype=torch.half)
    for k in range(hid // 16):
        w_sel = w.clone()
        sel = torch.zeros(16, hid, device='cuda', dtype=torch.half)
        sel[torch.arange(16), 16 * k + torch.arange(16)] = 1
        w_sel[hid * (din + hid):] = sel.view(-1)
        y = torch.empty(B, 16, device='cuda', dtype=torch.half)
        capi.check(capi.lib.ngp_ffmlp_inference_ex(x.data_ptr(), w_sel.data_ptr(), B, din, 16, hid, nl, 0, 6, None, y.data_ptr(), 0, capi.stream()))
        act[:, 16 * k:16 * (k + 1)] = y
    # (the selected layer is hidden layer 1, the one below the output layer: W_in and the hidden matmul are those of w)
    _, _, bb = _backward(B, din, hid, nl, capi.NGP_FF_DEFER_REDUCE)
    slabs = _slabs(bb, B, din, hid, nl)
    n_slabs = slabs.shape[0]
    assert n_slabs > 1
    tiles = torch.arange(B // 32, device='cuda')
    owner = (tiles // 4) % n_slabs   # workgroup b takes tiles 4 b .. 4 b + 3 of every round of 4 n_slabs tiles
    rounds = 0
    for b in range(0, n_slabs, max(1, n_slabs // 8)):
        rows = (tiles[owner == b][:, None] * 32 + torch.arange(32, device='cuda')[None]).view(-1)
        want = dy[rows].double().t() @ act[rows].double()          # [16, hid]
        got = slabs[b, hid * (din + hid):].view(16, hid).double()
        # n fp32 additions of terms t: |error| <= n 2^-24 sum |t| to first order; twice that as the bar
        bar = rows.numel() * 2.0 ** -23 * float((dy[rows].double().abs().t() @ act[rows].double().abs()).max())
        assert float((got - want).abs().max()) <= bar
        rounds += int((got != want).sum())
    assert rounds > 0
