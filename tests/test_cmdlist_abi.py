"""CPU checks of the native command list's C entries (include/ngp_hip.h ngp_cmdlist_*): every refusal, word for word, before any device
work; and that every launch site of the library goes through the recording helpers of csrc/common.h.  The packing itself runs under the
host sanitizers in tools/cmdlist_selftest.cpp (a stand-alone program, no Python)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_OR_DESTROYED = 'ngp_cmdlist_{}: the list is NULL or was destroyed'


@pytest.fixture()
def lib():
    import _ngp_capi as capi
    return capi.lib


def _create(lib):
    h = ctypes.c_void_p()
    assert lib.ngp_cmdlist_create(ctypes.byref(h)) == 0 and h.value
    return h.value


def _refused(lib, rc, message):
    assert rc == 1 and lib.ngp_last_error().decode() == message, (rc, lib.ngp_last_error())


def _count(lib, h):
    n = ctypes.c_uint32(99)
    rc = lib.ngp_cmdlist_count(h, ctypes.byref(n))
    return rc, n.value


def test_null_list_is_refused_by_every_entry(lib):
    n, buf = ctypes.c_uint32(), ctypes.create_string_buffer(16)
    _refused(lib, lib.ngp_cmdlist_create(None), 'ngp_cmdlist_create: out_list is NULL')
    _refused(lib, lib.ngp_cmdlist_begin(None), NULL_OR_DESTROYED.format('begin'))
    _refused(lib, lib.ngp_cmdlist_mark(None, 1, -1), NULL_OR_DESTROYED.format('mark'))
    _refused(lib, lib.ngp_cmdlist_end(None), NULL_OR_DESTROYED.format('end'))
    _refused(lib, lib.ngp_cmdlist_count(None, ctypes.byref(n)), NULL_OR_DESTROYED.format('count'))
    _refused(lib, lib.ngp_cmdlist_entry_name(None, 0, buf, 16), NULL_OR_DESTROYED.format('entry_name'))
    _refused(lib, lib.ngp_cmdlist_replay(None, None), NULL_OR_DESTROYED.format('replay'))
    _refused(lib, lib.ngp_cmdlist_wait_mark(None, 1, None), NULL_OR_DESTROYED.format('wait_mark'))
    _refused(lib, lib.ngp_cmdlist_destroy(None), NULL_OR_DESTROYED.format('destroy'))


def test_empty_list_counts_zero_and_is_not_replayed(lib):
    h = _create(lib)
    assert _count(lib, h) == (0, 0)
    _refused(lib, lib.ngp_cmdlist_replay(h, None), 'ngp_cmdlist_replay: the list is empty')
    _refused(lib, lib.ngp_cmdlist_wait_mark(h, 3, None), 'ngp_cmdlist_wait_mark: mark 3 was never recorded')
    _refused(lib, lib.ngp_cmdlist_entry_name(h, 0, ctypes.create_string_buffer(16), 16),
             'ngp_cmdlist_entry_name: index 0 is past the end of the list (0 entries)')
    assert lib.ngp_cmdlist_destroy(h) == 0


def test_begin_end_pairing_and_open_lists(lib):
    a, b = _create(lib), _create(lib)
    _refused(lib, lib.ngp_cmdlist_end(a), 'ngp_cmdlist_end: no recording is open on this thread')
    assert lib.ngp_cmdlist_begin(a) == 0
    _refused(lib, lib.ngp_cmdlist_begin(b), 'ngp_cmdlist_begin: a recording is already open on this thread')
    _refused(lib, lib.ngp_cmdlist_begin(a), 'ngp_cmdlist_begin: a recording is already open on this thread')
    _refused(lib, lib.ngp_cmdlist_end(b), 'ngp_cmdlist_end: another list is recording on this thread')
    _refused(lib, lib.ngp_cmdlist_replay(a, None), 'ngp_cmdlist_replay: the list is still recording')
    _refused(lib, lib.ngp_cmdlist_wait_mark(a, 1, None), 'ngp_cmdlist_wait_mark: the list is still recording')
    _refused(lib, lib.ngp_cmdlist_destroy(a), 'ngp_cmdlist_destroy: the list is still recording')
    assert lib.ngp_cmdlist_mark(a, 7, -1) == 0          # a mark at the (empty) list's end
    _refused(lib, lib.ngp_cmdlist_mark(a, 7, -1), 'ngp_cmdlist_mark: mark 7 exists already')
    _refused(lib, lib.ngp_cmdlist_mark(a, 8, 1), 'ngp_cmdlist_mark: position 1 is past the end of the list')
    assert lib.ngp_cmdlist_end(a) == 0
    _refused(lib, lib.ngp_cmdlist_end(a), 'ngp_cmdlist_end: no recording is open on this thread')
    _refused(lib, lib.ngp_cmdlist_begin(a), 'ngp_cmdlist_begin: the list has been recorded already (a list is recorded once)')
    # closed and empty: a recorded mark is found, then the list is refused as empty; an unknown mark is refused as such
    _refused(lib, lib.ngp_cmdlist_wait_mark(a, 7, None), 'ngp_cmdlist_wait_mark: the list is empty')
    _refused(lib, lib.ngp_cmdlist_wait_mark(a, 8, None), 'ngp_cmdlist_wait_mark: mark 8 was never recorded')
    _refused(lib, lib.ngp_cmdlist_replay(a, None), 'ngp_cmdlist_replay: the list is empty')
    assert _count(lib, a) == (0, 0)
    assert lib.ngp_cmdlist_begin(b) == 0 and lib.ngp_cmdlist_end(b) == 0   # the thread records again after `a` closed
    assert lib.ngp_cmdlist_destroy(a) == 0 and lib.ngp_cmdlist_destroy(b) == 0


def test_an_entry_that_fails_while_recording_leaves_the_list_unusable(lib):
    import _ngp_capi as capi
    h = _create(lib)
    assert lib.ngp_cmdlist_begin(h) == 0
    one = ctypes.c_void_p(16)   # never dereferenced: the entry's validation fails first
    assert lib.ngp_sh_encode_forward(one, one, 8, 3, 9, None, capi.NGP_F32, None) == 1 and b'degree in [1, 8]' in lib.ngp_last_error()
    assert lib.ngp_cmdlist_end(h) == 0
    _refused(lib, lib.ngp_cmdlist_replay(h, None), 'ngp_cmdlist_replay: the list is unusable: an entry failed while it was recording')
    assert lib.ngp_cmdlist_destroy(h) == 0
    # a refusal of the list's own entries does not poison the list that records
    a, b = _create(lib), _create(lib)
    assert lib.ngp_cmdlist_begin(a) == 0
    _refused(lib, lib.ngp_cmdlist_begin(b), 'ngp_cmdlist_begin: a recording is already open on this thread')
    assert lib.ngp_cmdlist_end(a) == 0
    _refused(lib, lib.ngp_cmdlist_replay(a, None), 'ngp_cmdlist_replay: the list is empty')
    assert lib.ngp_cmdlist_destroy(a) == 0 and lib.ngp_cmdlist_destroy(b) == 0


def test_double_destroy_and_use_after_destroy_are_refused(lib):
    h = _create(lib)
    assert lib.ngp_cmdlist_destroy(h) == 0
    _refused(lib, lib.ngp_cmdlist_destroy(h), NULL_OR_DESTROYED.format('destroy'))
    _refused(lib, lib.ngp_cmdlist_begin(h), NULL_OR_DESTROYED.format('begin'))
    _refused(lib, lib.ngp_cmdlist_replay(h, None), NULL_OR_DESTROYED.format('replay'))
    assert _count(lib, h)[0] == 1


def test_python_wrapper_refuses_a_destroyed_list():
    from cmdlist import CommandList
    cl = CommandList()
    assert cl.count() == 0 and cl.names() == []
    cl.destroy()
    cl.destroy()   # (idempotent on the wrapper: the handle is forgotten)
    with pytest.raises(RuntimeError, match='NULL or was destroyed'):
        cl.replay(None)


def test_every_launch_site_goes_through_the_recording_helpers():
    """csrc/common.h owns the only calls that put work on a stream; a launch site that bypassed it would escape every command list"""
    raw = re.compile(r'\b(hipLaunchKernelGGL|hipLaunchKernel|hipMemsetAsync|hipMemcpyAsync|hipModuleLaunchKernel|hipExtLaunchKernel)\s*\(|<<<')
    src = os.path.join(ROOT, 'torch-ngp_amd', 'csrc')
    allowed = {'common.h': 3, 'cmdlist.cpp': 3}   # the helpers themselves; the list's replay
    seen, sites = {}, 0
    for path in sorted(glob.glob(os.path.join(src, '*'))):
        if not path.endswith(('.hip', '.cpp', '.h', '.inc')):
            continue
        text = re.sub(r'//[^\n]*', '', open(path).read())
        n = len(raw.findall(text))
        if n:
            seen[os.path.basename(path)] = n
        sites += len(re.findall(r'\bNGP_LAUNCH(?:_STATUS)?\(|\b[A-Z0-9]+_LAUNCH_1D\(|memset_async\(|memcpy_async\(', text))
    assert seen == allowed, seen
    assert sites >= 100
