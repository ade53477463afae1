"""CPU checks of the mesh extraction entries (include/ngp_hip.h ngp_surface_nets_workspace_bytes / _count / _emit, ngp_lattice_points and its
workspace query; raymarching.surface_nets / lattice_points / lattice_frame; NeRFRenderer.extract_mesh; nerf.utils.save_mesh; DESIGN.md
3.17): declared, exported and bound; host-side validation returns the documented error without a device; the workspace sizes; the built
kernels neither spill nor use atomics; the PLY writer round-trips."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ngp_surface_nets_count': 9, 'ngp_surface_nets_emit': 18, 'ngp_lattice_points': 21}
QUERIES = ('ngp_surface_nets_workspace_bytes', 'ngp_lattice_points_workspace_bytes')


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name, n_params in ENTRIES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert fn.argtypes == capi._SIGNATURES[name] and fn.restype == ctypes.c_int and len(fn.argtypes) == n_params
    for name in QUERIES:
        assert re.search(r'\bsize_t\s+' + name + r'\s*\(', text)
        assert name in capi.EXPORTED and getattr(capi.lib, name).restype == ctypes.c_size_t
    block = text[text.index('mesh extraction: naive surface nets'):text.index('size_t ngp_surface_nets_workspace_bytes(')]
    for phrase in ('inside iff s > 0', 't = s_a / (s_a - s_b) clamped to [0, 1]', 'q0 = p - e_b - e_c', '(linear lattice index of p) * 3 + a', 'truncated'):
        assert phrase in block, phrase
    # additive entries: the version every existing caller checks stays
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_python_surface_is_exported():
    import raymarching
    from nerf.renderer import NeRFRenderer
    from nerf.network_sdf import NeuSNetwork
    from nerf import utils
    for name in ('surface_nets', 'lattice_points', 'lattice_frame'):
        assert name in raymarching.raymarching.__all__ and callable(getattr(raymarching, name))
    assert callable(NeRFRenderer.extract_mesh) and callable(utils.save_mesh)
    assert (NeRFRenderer.mesh_level, NeRFRenderer.mesh_inside_below, NeRFRenderer.mesh_fill) == (10.0, False, 0.0)
    assert (NeuSNetwork.mesh_level, NeuSNetwork.mesh_inside_below, NeuSNetwork.mesh_fill) == (0.0, True, 1.0)


def _emit_args(vol, dims, ws, verts, v_cap, faces, f_cap):
    return (vol, *dims, 0.0, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, ws, verts, v_cap, faces, f_cap, None)


def test_surface_nets_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)   # never dereferenced: validation fails first
    count, emit = lib.ngp_surface_nets_count, lib.ngp_surface_nets_emit
    # null pointers
    for i in range(3):           # volume, workspace, counts
        p = [one] * 3
        p[i] = None
        assert count(p[0], 8, 8, 8, 0.0, 0, p[1], p[2], None) == 1 and b'surface_nets_count: NULL' in lib.ngp_last_error(), i
    for i in range(4):           # volume, workspace, vertices, faces
        p = [one] * 4
        p[i] = None
        assert emit(*_emit_args(p[0], (8, 8, 8), p[1], p[2], 16, p[3], 16)) == 1 and b'surface_nets_emit: NULL' in lib.ngp_last_error(), i
    # a dimension below 2
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8)):
        assert count(one, *dims, 0.0, 0, one, one, None) == 1 and b'at least 2' in lib.ngp_last_error()
        assert emit(*_emit_args(one, dims, one, one, 16, one, 16)) == 1 and b'at least 2' in lib.ngp_last_error()
        assert lib.ngp_surface_nets_workspace_bytes(*dims) == 0
    # nx * ny * nz >= 2^31
    for dims in ((2048, 1024, 1024), (1 << 16, 1 << 16, 2), (1290, 1291, 1290)):
        assert count(one, *dims, 0.0, 0, one, one, None) == 1 and b'below 2^31' in lib.ngp_last_error()
        assert emit(*_emit_args(one, dims, one, one, 16, one, 16)) == 1 and b'below 2^31' in lib.ngp_last_error()
        assert lib.ngp_surface_nets_workspace_bytes(*dims) == 0
    # zero capacities
    assert emit(*_emit_args(one, (8, 8, 8), one, one, 0, one, 16)) == 1 and b'zero capacity' in lib.ngp_last_error()
    assert emit(*_emit_args(one, (8, 8, 8), one, one, 16, one, 0)) == 1 and b'zero capacity' in lib.ngp_last_error()
    with pytest.raises(RuntimeError, match='zero capacity'):
        capi.check(emit(*_emit_args(one, (8, 8, 8), one, one, 0, one, 0)))


def test_lattice_points_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)

    def call(nx=8, ny=8, z0=0, z1=8, bits=one, bound=1.0, C=1, H=128, dilate=1, ws=one, points=one, index=one, count=one, capacity=512):
        return lib.ngp_lattice_points(-1.0, -1.0, -1.0, 0.25, 0.25, 0.25, nx, ny, z0, z1, bits, bound, C, H, dilate, ws, points, index, count, capacity, None)
    for name in ('ws', 'points', 'index', 'count'):
        assert call(**{name: None}) == 1 and b'lattice_points: NULL' in lib.ngp_last_error(), name
    for kw in (dict(nx=0), dict(ny=0), dict(z0=4, z1=4), dict(z0=5, z1=4)):
        assert call(**kw) == 1 and b'empty lattice' in lib.ngp_last_error(), kw
    assert call(nx=1 << 16, ny=1 << 15, z1=1) == 1 and b'below 2^31' in lib.ngp_last_error()
    assert call(nx=1 << 12, ny=1 << 12, z0=127, z1=128) == 1 and b'below 2^31' in lib.ngp_last_error()
    assert call(capacity=0) == 1 and b'zero capacity' in lib.ngp_last_error()
    for kw, msg in ((dict(bound=0.0), b'bound'), (dict(bound=float('nan')), b'bound'), (dict(C=0), b'cascade'), (dict(C=9), b'cascade'),
                    (dict(H=0), b'grid_size'), (dict(H=2048), b'grid_size'), (dict(H=100), b'power of two'), (dict(dilate=5), b'dilate')):
        assert call(**kw) == 1 and msg in lib.ngp_last_error(), kw
    assert lib.ngp_lattice_points_workspace_bytes(0, 8, 8) == 0 and lib.ngp_lattice_points_workspace_bytes(1 << 12, 1 << 12, 128) == 0


def test_workspace_sizes_are_monotone_and_cover_the_map():
    import _ngp_capi as capi
    ws = lambda nx, ny, nz: int(capi.lib.ngp_surface_nets_workspace_bytes(nx, ny, nz))
    assert ws(2, 2, 2) >= 4 * 8
    for base in ((2, 2, 2), (5, 3, 130), (17, 9, 33), (129, 129, 129), (512, 512, 512)):
        nx, ny, nz = base
        n = nx * ny * nz
        blocks = -(-n // 256)
        assert ws(*base) >= 4 * n + 8 * blocks                       # the int32 map, one word per lattice point, and two scan words per workgroup
        assert ws(*base) <= 4 * n + 8 * blocks + 8 + 256              # ... the two totals and the map's padding, nothing more
        assert ws(nx + 1, ny, nz) >= ws(*base) and ws(nx, ny + 1, nz) >= ws(*base) and ws(nx, ny, nz + 1) >= ws(*base)
    sizes = [ws(n, n, n) for n in range(2, 40)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    lp = lambda nx, ny, nz: int(capi.lib.ngp_lattice_points_workspace_bytes(nx, ny, nz))
    assert lp(1, 1, 1) == 8 and lp(16, 16, 1) == 8 and lp(16, 16, 2) == 12 and lp(256, 256, 256) == 4 * (65536 + 1)


def test_lattice_frame_narrows_once():
    import raymarching
    o, h = raymarching.lattice_frame(-1, 1, (96, 5, 2))
    assert o == [-1.0, -1.0, -1.0] and h == [float(np.float32(2.0 / 95.0)), 0.5, 2.0]
    o, h = raymarching.lattice_frame((-1.0, 0.1, 0.0), (1.0, 0.7, 0.0), (4, 4, 1))
    assert o[1] == float(np.float32(0.1)) and h[1] == float(np.float32((0.7 - 0.1) / 3.0)) and h[2] == 0.0
    import surface_nets_cases as sn
    o2, h2 = sn.lattice_spacing((-1.0, 0.1, 0.0), (1.0, 0.7, 1.0), (4, 4, 3))
    o3, h3 = raymarching.lattice_frame((-1.0, 0.1, 0.0), (1.0, 0.7, 1.0), (4, 4, 3))
    assert o2.tolist() == o3 and h2.tolist() == h3                   # the model's frame is the wrapper's


def test_extract_mesh_refuses_a_cull_without_cuda_ray():
    from nerf.renderer import NeRFRenderer
    m = NeRFRenderer(bound=1, cuda_ray=False)
    with pytest.raises(RuntimeError, match='cuda_ray'):
        m.extract_mesh(resolution=8)
    with pytest.raises(ValueError, match='resolution'):
        m.extract_mesh(resolution=1, cull=False)


def _read_ply(path):
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    header = raw[:end].decode('ascii').splitlines()
    assert header[0] == 'ply' and header[1] == 'format binary_little_endian 1.0'
    n_vertices = int(next(line for line in header if line.startswith('element vertex')).split()[-1])
    n_faces = int(next(line for line in header if line.startswith('element face')).split()[-1])
    props = [line.split()[-1] for line in header if line.startswith('property float')]
    assert 'property list uchar int vertex_indices' in header
    v = np.frombuffer(raw, '<f4', n_vertices * len(props), end).reshape(n_vertices, len(props))
    rows = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), n_faces, end + v.nbytes)
    assert end + v.nbytes + rows.nbytes == len(raw)
    return props, v, rows


@pytest.mark.parametrize('with_normals', [False, True])
def test_ply_round_trip(tmp_path, with_normals):
    import surface_nets_cases as sn
    from nerf.utils import save_mesh
    v64, f = sn.surface_nets(sn.noise((6, 7, 8)), 0.5, origin=(-1.0, 0.5, 2.0), spacing=(0.25, 0.5, 1.0))
    v = v64.astype(np.float32)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    path = str(tmp_path / 'mesh.ply')
    save_mesh(path, torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n))
    props, got_v, rows = _read_ply(path)
    assert props == ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if with_normals else [])
    assert np.array_equal(got_v[:, :3], v) and (not with_normals or np.array_equal(got_v[:, 3:], n))
    assert (rows['n'] == 3).all() and np.array_equal(rows['v'], f)
    # an empty mesh is a valid file; a face that names a missing vertex is refused
    save_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    props, got_v, rows = _read_ply(path)
    assert len(got_v) == 0 and len(rows) == 0
    with pytest.raises(ValueError, match='does not exist'):
        save_mesh(path, v[:3], np.array([[0, 1, 3]], np.int32))


@pytest.mark.parametrize('build', ['_obj', '_obj_dbg'])
def test_new_unit_neither_spills_nor_uses_atomics(build, tmp_path):
    """read off the built object: seven kernels, no scratch, no atomics of any kind (the output order is the scans' order), and no 64-bit
    shift with its amount in the last allocated register (tools/check_isa_hazards.py)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    obj = os.path.join(ROOT, 'torch-ngp_amd', 'csrc', build, 'surface_nets.o')
    if not os.path.exists(obj) or not isa.tools_present():
        pytest.skip(f'{obj} (run __graft_entry__.build()) or the LLVM tools are missing')
    checked, hits = isa.scan_object(obj)
    assert checked == 7 and hits == []
    co = isa.code_object(obj, str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    names = sorted(re.search(r'k_(surface_nets_[a-z]+|lattice_[a-z]+|scan_partialsILi\d)', k).group(1) for k in meta)
    assert names == ['lattice_count', 'lattice_emit', 'scan_partialsILi1', 'scan_partialsILi2', 'surface_nets_count', 'surface_nets_faces',
                     'surface_nets_vertices']
    for k, m in meta.items():
        assert m['private_segment_fixed_size'] == 0 and m['vgpr_count'] <= 64, (k, m)
        assert not any(i.startswith('scratch_') or '_atomic' in i or i.startswith('ds_add') for i in kernels[k]), k
