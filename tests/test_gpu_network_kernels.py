"""GPU checks of the fused network kernels at the C ABI (include/ngp_hip.h): ngp_network_forward / ngp_network_forward_rows,
ngp_network_backward_color, ngp_ffmlp_backward_ex with NGP_FF_INPUT_PLANAR | NGP_FF_DX_PLANAR (plus NGP_FF_DEFER_REDUCE, NGP_FF_RECOMPUTE),
ngp_ffmlp_reduce_slabs_pair, the four glue kernels of csrc/pipeline.hip, ngp_pipeline_mse_loss and ngp_pad_2d_fp16 -- against the float64
model, the cases and the criteria of tests/network_cases.py (tests/test_network_cases.py proves on the CPU that the float32 twin of the
model meets every criterion and that every deliberately wrong variant fails one).

Every model stage is evaluated from the GPU's own stored upstream tensors (h16, color_in, g_h16), outputs are prefilled with NaN or a
sentinel, and every test prints its report (criterion, observed figure, bar) before it asserts (pytest -s); EXPERIMENTS.md has the table."""
import numpy as np
import pytest
import torch

import network_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 123.25


def _capi():
    import _ngp_capi as capi
    return capi


def cu16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().half()


def cu32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def p(t):
    return None if t is None else t.data_ptr()


def full(shape, value, dtype=torch.half):
    return torch.full(shape, value, device='cuda', dtype=dtype)


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int16 if a.dtype == torch.half else torch.int32
    return torch.equal(a.view(view), b.view(view))


def _m_big():
    """the smallest multiple of 128 whose tile count exceeds one trip of ngp_network_forward_rows' grid: the launch has at most
    CUs x NGP_NETFWD_PER_CU (4) workgroups of 4 waves, every wave iteration takes one tile of 32 rows, so more than 4 * CUs * 4 tiles
    (131200 rows on 256 CUs) send the grid-stride loop and its one-group-ahead request() on a second trip"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (4 * cus * 4 * 32) // 128 * 128 + 128


def _upload(case):
    return dict(enc=cu16(case['enc']), enc_planar=cu16(case['enc_planar']), dirs=cu32(case['dirs']), ws=cu16(case['w_sigma']), wc=cu16(case['w_color']),
                g_out16=cu16(case['g_out16']), g_sigma=cu32(case['g_sigma']))


def _forward(dev, case, planar=True, training=True, buffers=True, rows=None, fill=float('nan'), use_rows_entry=False):
    """one launch of ngp_network_forward (rows / use_rows_entry: ngp_network_forward_rows) into outputs prefilled with `fill`"""
    capi = _capi()
    M, nl_s, nl_c = case['M'], case['nl_s'], case['nl_c']
    assert M % 128 == 0 and dev['dirs'].shape[0] == case['M_valid']
    o = dict(sigma=full((M,), fill, torch.float32), rgb=full((M, 3), fill, torch.float32))
    if training:
        o.update(h16=full((M, 16), fill), color_in=full((M, 32), fill))
        if buffers:
            o.update(fb_s=full((nl_s, M, 64), fill), fb_c=full((nl_c, M, 64), fill))
    enc = dev['enc_planar'] if planar else dev['enc']
    flags = capi.NGP_FF_INPUT_PLANAR if planar else 0
    args = (enc.data_ptr(), dev['dirs'].data_ptr(), M, case['M_valid'], dev['ws'].data_ptr(), dev['wc'].data_ptr(), nl_s, nl_c, C.DS_FORWARD,
            int(training), p(o.get('fb_s')), p(o.get('h16')), o['sigma'].data_ptr(), p(o.get('color_in')), p(o.get('fb_c')), o['rgb'].data_ptr(), flags)
    if rows is not None or use_rows_entry:
        capi.check(capi.lib.ngp_network_forward_rows(*args, p(rows), capi.stream()))
    else:
        capi.check(capi.lib.ngp_network_forward(*args, capi.stream()))
    torch.cuda.synchronize()
    return o


def _check(rep, what):
    print(f'\n{what}\n{rep}')
    assert not rep.failures(), (what, rep.failures())


def _wide_holds(case):
    if case['power']:
        w = C.wide_conditions(case, backward=False)
        assert w['below'] >= 0.02 and w['above'] >= 0.02 and w['h0_max'] < 80 and w['g0_max'] < 65504, w


# ------------------------------------------------------------------------------------------------
# a. the fused forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planar', [True, False], ids=['PLANAR', 'row-major'])
@pytest.mark.parametrize('kind', ['nominal', 'wide_h0'])
@pytest.mark.parametrize('M', [128, 4224, 'M_big'])
@pytest.mark.parametrize('nl_s,nl_c', [(2, 2), (2, 3), (3, 2), (4, 4)])
def test_fused_forward_against_the_float64_model(nl_s, nl_c, M, kind, planar):
    """training variant (both enc layouts: NGP_FF_INPUT_PLANAR and row-major): h16 against sigma_stage; sigma, the SH block, the shuffle, the
    pad and SH(0) behind M_valid against mid_forward(GPU h16); rgb against rgb_forward(color_stage(GPU color_in)) with the MLP bar carried
    through the sigmoid; rgb == half(rgb).  The inference variant and the training variant without forward buffers: the same bits."""
    M = _m_big() if M == 'M_big' else M
    case = C.CASES[kind](nl_s, nl_c, M)
    _wide_holds(case)
    dev = _upload(case)
    o = _forward(dev, case, planar)
    got = {k: host(o[k]) for k in ('h16', 'color_in', 'rgb')}
    got['sigma'] = o['sigma'].cpu().numpy()
    _check(C.forward_criteria(got, case), f'forward {kind} ({nl_s},{nl_c}) M={M} {"planar" if planar else "row-major"}')
    assert torch.isfinite(o['fb_s'].float()).all() and torch.isfinite(o['fb_c'].float()).all()          # every stored activation written
    inf = _forward(dev, case, planar, training=False)
    assert _same_bits(inf['sigma'], o['sigma']) and _same_bits(inf['rgb'], o['rgb'])
    nob = _forward(dev, case, planar, buffers=False)
    for k in ('sigma', 'rgb', 'h16', 'color_in'):
        assert _same_bits(nob[k], o[k]), k


# ------------------------------------------------------------------------------------------------
# b. ngp_network_forward_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('training', [False, True], ids=['inference', 'training'])
def test_forward_rows_stops_at_the_device_row_count(training):
    """rows below 32 * ceil(r / 32) (capped at M: k_network_forward takes min(n_tiles_cap, ceil(r / 32)) tiles) equal the rows_dev = NULL
    launch bit for bit, every row above keeps its sentinel in ALL outputs.  The stored activations are kept per tile of 32 rows
    ([layer][tile][2048] halves, layer_stride = tiles * NKB * 64 half8 units), so they are compared tile by tile."""
    M = 4224
    case = C.nominal(2, 3, M)
    dev = _upload(case)
    base = _forward(dev, case, training=training, fill=SENTINEL, use_rows_entry=True)
    for k, v in base.items():
        assert not bool((v == SENTINEL).any()), k                          # rows_dev = NULL: everything written
    for r in (0, 1, 32, 33, M - 31, M, M + 1000):
        rows = torch.tensor([r], dtype=torch.int64).to(torch.int32).cuda()      # (a uint32 device word)
        o = _forward(dev, case, training=training, rows=rows, fill=SENTINEL)
        lim = min(M, (r + 31) // 32 * 32)
        for k, v in o.items():
            if k in ('fb_s', 'fb_c'):
                v, b = v.view(v.shape[0], M // 32, 2048), base[k].view(v.shape[0], M // 32, 2048)
                assert _same_bits(v[:, :lim // 32], b[:, :lim // 32]), (r, k)
                assert bool((v[:, lim // 32:] == SENTINEL).all()), (r, k)
            else:
                assert _same_bits(v[:lim], base[k][:lim]), (r, k)
                assert bool((v[lim:] == SENTINEL).all()), (r, k)


# ------------------------------------------------------------------------------------------------
# c. the fused backward
# ------------------------------------------------------------------------------------------------
def _m_slabs(nl):
    capi = _capi()
    assert capi.lib.ngp_ffmlp_backward_slab_count(128, 32, 64, nl) == 0        # one workgroup: direct store
    M = 256
    while capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, nl) <= 1:
        M += 128
        assert M <= 8192
    return M


def _backward(dev, case, fwd, flags, g_h16_in=None):
    """ngp_network_backward_color -> ngp_ffmlp_backward_ex (planar in, planar dL/dx) -> (deferred) ngp_ffmlp_reduce_slabs_pair, on the stored
    forward `fwd`; in the wide_h0 case the sigma net is fed g_h16 with column 0 times 2**-shift (network_cases.wide_h0)"""
    capi = _capi()
    st = capi.stream()
    M, nl_s, nl_c = case['M'], case['nl_s'], case['nl_c']
    nan = float('nan')
    recompute = bool(flags & capi.NGP_FF_RECOMPUTE)
    fb_s, fb_c = (None, None) if recompute else (fwd['fb_s'], fwd['fb_c'])
    scratch_c, scratch_s = full((nl_c, M, 64), 0.0), full((nl_s, M, 64), 0.0)
    o = dict(g_h16=full((M, 16), nan), g_wc=full((C.n_params(nl_c),), nan), g_ws=full((C.n_params(nl_s),), nan), g_enc=full((16, M, 2), nan))
    capi.check(capi.lib.ngp_network_backward_color(dev['g_out16'].data_ptr(), fwd['color_in'].data_ptr(), dev['wc'].data_ptr(), p(fb_c), M, nl_c,
                                                   scratch_c.data_ptr(), dev['g_sigma'].data_ptr(), fwd['h16'].data_ptr(), C.DS_BACKWARD,
                                                   o['g_h16'].data_ptr(), o['g_wc'].data_ptr(), flags, st))
    fed = o['g_h16']
    if case['shift']:
        fed = o['g_h16'].clone()
        fed[:, 0] = (o['g_h16'][:, 0].float() * 2.0 ** -case['shift']).half()
    capi.check(capi.lib.ngp_ffmlp_backward_ex(fed.data_ptr(), dev['enc_planar'].data_ptr(), dev['ws'].data_ptr(), p(fb_s), M, 32, 16, 64, nl_s, 0, 6, 1,
                                              scratch_s.data_ptr(), o['g_enc'].data_ptr(), o['g_ws'].data_ptr(),
                                              capi.NGP_FF_INPUT_PLANAR | capi.NGP_FF_DX_PLANAR | flags, st))
    if flags & capi.NGP_FF_DEFER_REDUCE:
        n_c, n_s = capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, nl_c), capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, nl_s)
        capi.check(capi.lib.ngp_ffmlp_reduce_slabs_pair(scratch_c.data_ptr(), n_c, o['g_wc'].numel(), o['g_wc'].data_ptr(), scratch_s.data_ptr(), n_s,
                                                        o['g_ws'].numel(), o['g_ws'].data_ptr(), None, st))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('kind', ['nominal', 'wide_h0'])
@pytest.mark.parametrize('M', [128, 'slabs', 33408])
@pytest.mark.parametrize('nl_s,nl_c', [(2, 2), (2, 3), (3, 2), (3, 3)])
def test_fused_backward_against_the_float64_model(nl_s, nl_c, M, kind):
    """column 0 of g_h16 against mid_backward(GPU h16) (density_scale 1.3; wide_h0: the clamp at +-15 on both sides), columns 1..15 and g_wc
    against color_backward(GPU color_in), the PLANAR g_enc (NGP_FF_DX_PLANAR, from the NGP_FF_INPUT_PLANAR input) and g_ws against
    sigma_backward(GPU g_h16) -- for the direct store (M = 128), the smallest M that leaves slabs, and 33408.  flags 0, NGP_FF_DEFER_REDUCE and
    NGP_FF_DEFER_REDUCE | NGP_FF_RECOMPUTE give the same bits (test_gpu_pipeline.py asserts that at length; one line of it here)."""
    capi = _capi()
    if M == 'slabs':
        M = max(_m_slabs(nl_s), _m_slabs(nl_c))
        assert min(capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, nl) for nl in (nl_s, nl_c)) > 1
    case = C.CASES[kind](nl_s, nl_c, M)
    _wide_holds(case)
    dev = _upload(case)
    fwd = _forward(dev, case)
    res = {flags: _backward(dev, case, fwd, flags) for flags in (0, capi.NGP_FF_DEFER_REDUCE, capi.NGP_FF_DEFER_REDUCE | capi.NGP_FF_RECOMPUTE)}
    got = {k: host(v) for k, v in res[0].items()}
    _check(C.backward_criteria(got, dict(h16=host(fwd['h16']), color_in=host(fwd['color_in'])), case), f'backward {kind} ({nl_s},{nl_c}) M={M}')
    for flags, o in res.items():
        assert all(_same_bits(o[k], res[0][k]) for k in o), flags


# ------------------------------------------------------------------------------------------------
# d. the glue kernels on the hand-written table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [None, 257])
def test_glue_kernels_on_the_table(rows):
    """ngp_pipeline_mid_forward / _mid_backward / _rgb_forward / _rgb_backward on glue_table() (every h0 around the clamp, +-inf, NaN,
    overflowing products, denormals) at the table's size and tiled to 257 rows (one full block and one lane of the next)"""
    capi = _capi()
    st = capi.stream()
    t = C.glue_table() if rows is None else C.tiled_table(rows)
    M = t['M']
    nan = float('nan')
    h16, dirs, out16 = cu16(t['h16']), cu32(t['dirs']), cu16(t['out16'])
    g_sigma, g_cin, g_rgb, rgb_in = cu32(t['g_sigma']), cu16(t['g_color_in']), cu32(t['g_rgb']), cu32(t['rgb'])
    assert np.array_equal(host(h16), t['h16'], equal_nan=True) and np.array_equal(g_sigma.cpu().numpy(), t['g_sigma'])
    sigma, color_in, rgb = full((M,), nan, torch.float32), full((M, 32), nan), full((M, 3), nan, torch.float32)
    g_out16, g_h16 = full((M, 16), nan), full((M, 16), nan)
    capi.check(capi.lib.ngp_pipeline_mid_forward(h16.data_ptr(), dirs.data_ptr(), sigma.data_ptr(), color_in.data_ptr(), M, M, C.DS_FORWARD, st))
    capi.check(capi.lib.ngp_pipeline_rgb_forward(out16.data_ptr(), rgb.data_ptr(), M, st))
    capi.check(capi.lib.ngp_pipeline_rgb_backward(g_rgb.data_ptr(), rgb_in.data_ptr(), g_out16.data_ptr(), M, st))
    capi.check(capi.lib.ngp_pipeline_mid_backward(g_sigma.data_ptr(), h16.data_ptr(), g_cin.data_ptr(), g_h16.data_ptr(), M, C.DS_BACKWARD, st))
    torch.cuda.synchronize()
    got = dict(sigma=sigma.cpu().numpy(), color_in=host(color_in), rgb=host(rgb), g_out16=host(g_out16), g_h16=host(g_h16))
    _check(C.glue_criteria(got, t), f'glue kernels, {M} rows')


@pytest.mark.parametrize('flags', [0, 'recompute'])
def test_backward_epilogue_on_the_table(flags):
    """the same h0 / g_sigma rows through the epilogue of ngp_network_backward_color (h16 is an input there: the table's column 0 and g_sigma
    replace the first rows of a nominal batch): column 0 against mid_backward by class and yardstick, and the same bits as
    ngp_pipeline_mid_backward -- a NaN h0 gives a NaN, not exp(-15)"""
    capi = _capi()
    st = capi.stream()
    flags = capi.NGP_FF_RECOMPUTE if flags == 'recompute' else 0
    t = C.glue_table()
    T = t['M']
    case = C.nominal(2, 2, 128)
    dev = _upload(case)
    fwd = _forward(dev, case)
    h16 = fwd['h16'].clone()
    h16[:T, 0] = cu16(t['h16'][:, 0])
    g_sigma = dev['g_sigma'].clone()
    g_sigma[:T] = cu32(t['g_sigma'])
    fwd = dict(fwd, h16=h16)
    o = _backward(dict(dev, g_sigma=g_sigma), case, fwd, flags)
    src = dict(h16=host(h16), g_sigma=g_sigma.cpu().numpy(), dirs=case['dirs'], M_valid=case['M_valid'])
    _check(C.glue_criteria(dict(g_h16=host(o['g_h16'])), src, only=('g_h16',)), 'epilogue of ngp_network_backward_color on the table rows')
    g_cin, ref = full((128, 32), 0.0), full((128, 16), float('nan'))
    capi.check(capi.lib.ngp_pipeline_mid_backward(g_sigma.data_ptr(), h16.data_ptr(), g_cin.data_ptr(), ref.data_ptr(), 128, C.DS_BACKWARD, st))
    torch.cuda.synchronize()
    assert _same_bits(o['g_h16'][:, 0].clone(), ref[:, 0].clone())
    nan_rows = np.flatnonzero(np.isnan(t['h16'][:, 0]))
    assert len(nan_rows) == len(C.G_SIGMA_VALUES) and bool(torch.isnan(o['g_h16'][nan_rows, 0].float()).all())


# ------------------------------------------------------------------------------------------------
# e. / f.
# ------------------------------------------------------------------------------------------------
def test_mse_loss_on_the_cases():
    """loss against the float64 mean by yardstick, grad_image bit for bit against (fl32(2) / fl32(n) * diff) * scale"""
    capi = _capi()
    rep = C.Report()
    for case in C.mse_cases():
        n = case['n']
        image, target = cu32(case['image']), cu32(case['target'])
        scale = None if case['scale'] is None else torch.tensor([case['scale']], device='cuda')
        loss, grad = full((1,), float('nan'), torch.float32), full((n,), float('nan'), torch.float32)
        capi.check(capi.lib.ngp_pipeline_mse_loss(image.data_ptr(), target.data_ptr(), n, p(scale), loss.data_ptr(), grad.data_ptr(), capi.stream()))
        torch.cuda.synchronize()
        ref, _ = C.mse_model(case['image'], case['target'], case['scale'], np.float64)
        _, want = C.mse_model(case['image'], case['target'], case['scale'], np.float32)
        bound, _ = C.yardstick('loss', case)
        err = abs(float(loss) - ref)
        rep.add(f'loss n={n} scale={case["scale"]}', err <= bound, err, bound)
        rep.add(f'grad_image n={n} scale={case["scale"]}', np.array_equal(grad.cpu().numpy().view(np.int32), want.view(np.int32)), 0, 'bits')
    _check(rep, 'ngp_pipeline_mse_loss')


def test_pad_2d_on_the_cases():
    capi = _capi()
    for (sr, sc, stride, dr, dc), src, want in C.pad_cases():
        s = cu16(src) if sr else None
        dst = full((dr, dc), SENTINEL)
        capi.check(capi.lib.ngp_pad_2d_fp16(p(s), sr, sc, stride, dst.data_ptr(), dr, dc, capi.stream()))
        torch.cuda.synchronize()
        assert np.array_equal(host(dst), want), (sr, sc, stride, dr, dc)
