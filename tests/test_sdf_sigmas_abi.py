"""CPU checks of the SDF density op (include/ngp_hip.h ngp_sdf_sigmas_forward / _backward / _workspace_bytes and the fp64 twins;
raymarching.sdf_sigmas; nerf.network_sdf.NeuSNetwork): declared, exported and bound; the ABI version unchanged; host-side
validation; the Python surface; the renderer hands the deltas to a model that asks for them and to no other (host logic on stand-ins)."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ngp_sdf_sigmas_forward': 9, 'ngp_sdf_sigmas_backward': 15, 'ngp_sdf_sigmas_forward_f64': 9, 'ngp_sdf_sigmas_backward_f64': 15}


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name, n_params in ENTRIES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert fn.argtypes == capi._SIGNATURES[name] and fn.restype == ctypes.c_int and len(fn.argtypes) == n_params
    assert re.search(r'\bsize_t\s+ngp_sdf_sigmas_workspace_bytes\s*\(\s*uint32_t M\s*\)', text)
    assert 'ngp_sdf_sigmas_workspace_bytes' in capi.EXPORTED and capi.lib.ngp_sdf_sigmas_workspace_bytes.restype == ctypes.c_size_t
    # the comment of the new block cites the rule it implements and the compositor statement it feeds
    block = text[text.index('signed-distance fields: NeuS'):text.index('size_t ngp_sdf_sigmas_workspace_bytes(')]
    assert 'NeuS' in block and 'raymarching.cu:501-577' in block and 'clip((prev - next + eps) / (prev + eps), 0, 1)' in block


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_pybind_table_is_untouched_and_the_op_is_exported():
    import raymarching
    assert 'sdf_sigmas' in raymarching.raymarching.__all__ and callable(raymarching.sdf_sigmas)
    from raymarching import backend
    assert callable(backend.sdf_sigmas_forward) and callable(backend.sdf_sigmas_backward)
    assert not hasattr(backend._backend, 'sdf_sigmas_forward')   # the reference's table of callables stays the reference's
    src = open(os.path.join(ROOT, 'torch-ngp_amd', 'csrc', 'bindings.cpp')).read()
    assert 'sdf_sigmas' not in src


def test_workspace_query():
    import _ngp_capi as capi
    ws = lambda m: int(capi.lib.ngp_sdf_sigmas_workspace_bytes(m))
    sizes = [ws(m) for m in (0, 1, 63, 64, 65, 256, 257, 1600, 262144, 262145, 1 << 31)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes)     # monotone in M
    assert ws(262144) == 8 * 1024 and ws(262145) == 8 * 1025            # one double per workgroup of 256 rows


def test_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    big = 1 << 20
    for suffix in ('', '_f64'):
        fwd, bwd = getattr(lib, 'ngp_sdf_sigmas_forward' + suffix), getattr(lib, 'ngp_sdf_sigmas_backward' + suffix)
        tag = suffix.encode()
        for i in range(6):   # sdf, normals, dirs, deltas, inv_s, sigmas
            p = [one] * 6
            p[i] = None
            assert fwd(*p[:5], 64, 1.0, p[5], None) == 1, (suffix, i)
            assert b'sdf_sigmas_forward' + tag + b': NULL tensor' in lib.ngp_last_error()
        for i in (0, 1, 2, 3, 4, 5, 6, 7, 9):   # everything but grad_dirs (8), which may be NULL; 10 is the workspace
            p = [one] * 10
            p[i] = None
            assert bwd(*p[:6], 64, 1.0, *p[6:], one, big, None) == 1, (suffix, i)
            assert b'sdf_sigmas_backward' + tag + b': NULL tensor' in lib.ngp_last_error()
        for bad in (-0.01, 1.01, float('nan')):
            assert fwd(*[one] * 5, 64, bad, one, None) == 1 and b'cos_anneal must be in [0, 1]' in lib.ngp_last_error()
            assert bwd(*[one] * 6, 64, bad, *[one] * 4, one, big, None) == 1 and b'cos_anneal must be in [0, 1]' in lib.ngp_last_error()
        need = int(lib.ngp_sdf_sigmas_workspace_bytes(1600))
        assert bwd(*[one] * 6, 1600, 1.0, *[one] * 4, one, need - 1, None) == 1 and b'workspace' in lib.ngp_last_error()
        assert bwd(*[one] * 6, 1600, 1.0, *[one] * 4, None, need, None) == 1 and b'workspace' in lib.ngp_last_error()
        # M == 0 is a no-op, whatever the pointers
        assert fwd(None, None, None, None, None, 0, 1.0, None, None) == 0
        assert bwd(*[None] * 6, 0, 1.0, None, None, None, None, None, 0, None) == 0
    with pytest.raises(RuntimeError, match='cos_anneal'):
        capi.check(lib.ngp_sdf_sigmas_forward(one, one, one, one, one, 64, 2.0, one, None))


@pytest.mark.parametrize('build', ['_obj', '_obj_dbg'])
def test_new_unit_is_streaming_code(build, tmp_path):
    """read off the built object: three kernels, no scratch, no LDS beyond the four cross-wave partials, no float atomics, and no 64-bit
    shift with its amount in the last allocated register (tools/check_isa_hazards.py)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    obj = os.path.join(ROOT, 'torch-ngp_amd', 'csrc', build, 'sdf_sigmas.o')
    if not os.path.exists(obj) or not isa.tools_present():
        pytest.skip(f'{obj} (run __graft_entry__.build()) or the LLVM tools are missing')
    checked, hits = isa.scan_object(obj)
    assert checked == 3 and hits == []
    co = isa.code_object(obj, str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    assert sorted(k.split('k_sdf_sigmas_')[1][:3] for k in meta) == ['bwd', 'fwd', 'inv']
    for k, m in meta.items():
        assert m['private_segment_fixed_size'] == 0 and m['vgpr_count'] <= 64, (k, m)
        assert not any(i.startswith('scratch_') or i.startswith('global_atomic') or i.startswith('ds_add') for i in kernels[k]), k


class _Recorder(torch.nn.Module):
    """what the renderer calls: records the arguments of forward"""

    def __init__(self, takes_deltas):
        super().__init__()
        if takes_deltas:
            self.takes_deltas = True
        self.calls = []

    def forward(self, *args, **kwargs):
        self.calls.append((len(args), sorted(kwargs)))
        raise _Called()


class _Called(Exception):
    pass


@pytest.mark.parametrize('takes_deltas', [False, True])
def test_stage_issuer_hands_the_deltas_to_a_model_that_asks_for_them(takes_deltas):
    """render_loop.StageIssuer.iteration on stand-ins: the march is a no-op, the model call is recorded and ends the iteration"""
    from nerf import render_loop
    model = _Recorder(takes_deltas)
    model.bound, model.cascade, model.grid_size, model.density_scale = 1.0, 1, 128, 1.0
    opt = types.SimpleNamespace(probe=None, iter_hook=None, scaled=False, takes_deltas=takes_deltas)
    rb = types.SimpleNamespace(march_rays_dev=lambda *a: None)
    frame = types.SimpleNamespace(model=model, rb=rb, opt=opt, state=[None, None], alive=[None, None], T_thresh=1e-2, dev='cpu', t=None, o=None,
                                  d=None, dt_gamma=0.0, max_steps=8, bits=None, near=None, far=None, aux_infer=None)
    issuer = render_loop.StageIssuer.__new__(render_loop.StageIssuer)
    issuer.f, issuer.rf, issuer.probe, issuer.tag = frame, None, None, None
    with pytest.raises(_Called):
        issuer.iteration(0, 4, 128, None, 4, 0)
    assert model.calls == [(2, ['deltas'] if takes_deltas else [])]


def test_loop_options_keep_a_deltas_model_off_the_native_path():
    from nerf.render_loop import LoopOptions
    plain = types.SimpleNamespace(grid_size=128, forward_scaled=lambda *a: None)
    assert LoopOptions(plain).read_policy().native is True and LoopOptions(plain).read_policy().takes_deltas is False
    sdf = types.SimpleNamespace(grid_size=128, forward_scaled=lambda *a: None, takes_deltas=True)
    opt = LoopOptions(sdf).read_policy()
    assert opt.native is False and opt.takes_deltas is True


def test_run_cuda_source_calls_the_model_both_ways():
    """the training branch and the eager eval loop of run_cuda: one call form per kind of model (read off the source: the branch needs a
    GPU to run; tests/test_gpu_network_sdf.py runs it)"""
    src = open(os.path.join(ROOT, 'torch-ngp_amd', 'nerf', 'renderer.py')).read()
    form = "self(xyzs, dirs, deltas=deltas) if getattr(self, 'takes_deltas', False) else self(xyzs, dirs)"
    assert src.count(form) == 2 and src.count('self(xyzs, dirs') == 4


def test_neus_network_constructs_on_the_cpu():
    from nerf.network_sdf import NeuSNetwork
    from nerf.renderer import NeRFRenderer
    m = NeuSNetwork(bound=1, cuda_ray=True, log2_hashmap_size=12, prior_radius=0.6)
    assert isinstance(m, NeRFRenderer) and m.takes_deltas is True and m.graph_loop is False and m.native_loop is False
    assert not hasattr(m, 'fused') and not hasattr(m, 'forward_scaled')   # the module-by-module branch everywhere
    shapes = {k: tuple(v.shape) for k, v in m.named_parameters()}
    assert set(shapes) == {'encoder.embeddings', 'sdf_net.weights', 'color_net.weights', 'log_inv_s'}
    assert shapes['log_inv_s'] == (1,) and shapes['sdf_net.weights'] == (64 * (32 + 64 + 16),) and shapes['color_net.weights'] == (64 * (32 + 64 + 16),)
    assert m.encoder.output_dim == 32 and m.sdf_net.output_dim == 16 and m.color_net.input_dim == 32 and m.encoder_dir.output_dim == 9
    assert abs(float(m.inv_s.detach()) - 20.0) < 1e-4 and m.cos_anneal == 1.0 and m.prior_radius == 0.6
    assert sum(len(list(g['params'])) for g in m.get_params(1e-2)) == 4
    assert 'No gradient is needed' in NeuSNetwork.density.__doc__
    with pytest.raises(ValueError, match='deltas'):
        m(torch.zeros(4, 3), torch.zeros(4, 3))
