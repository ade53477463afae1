"""No GPU: the row bound of the training chain at the C ABI (include/ngp_hip.h ngp_training_row_bound) -- the header, the ctypes table and the
exports agree; the refusals of an armed bound come before any device work; with nothing armed (NULL) the entries take the path they took
before; the bound belongs to the thread that armed it."""
import ctypes
import os
import re
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def lib():
    import _ngp_capi as capi
    yield capi.lib
    capi.lib.ngp_training_row_bound(None)


ONE = ctypes.c_void_p(16)    # never dereferenced: every call below is refused on the host


def test_header_ctypes_table_and_exports_agree():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+ngp_training_row_bound\s*\(\s*const\s+uint32_t\s*\*\s*rows_dev\s*\)\s*;', text)
    assert 'ngp_training_row_bound' in capi.EXPORTED and hasattr(capi.lib, 'ngp_training_row_bound')
    assert capi.lib.ngp_training_row_bound.argtypes == [ctypes.c_void_p] and capi.lib.ngp_training_row_bound.restype is ctypes.c_int
    # additive: the version stays, and no existing entry changed its signature (tests/test_capi_exports.py compares every prototype)
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def _mlp_backward(lib, capi, flags, num_layers=2, hidden=64):
    return lib.ngp_ffmlp_backward_ex(None, None, None, None, 128, 32, 16, hidden, num_layers, 0, 6, 1, None, None, None, flags, None)


def _grid_backward(lib, capi, dy_dx):
    return lib.ngp_grid_encode_backward_checked_slabs(None, None, None, None, None, 128, 3, 2, 2, 1.0, 4, dy_dx, dy_dx, 0, 0, 0, capi.NGP_F16, 0.0, None, None, 0,
                                                      None, None, None)


def test_an_armed_bound_is_refused_where_no_kernel_serves_it(lib):
    import _ngp_capi as capi
    assert lib.ngp_training_row_bound(ONE) == 0
    # the MLP backward: the paired kernel serves the bound, the single-wave and layered kernels and the 4-layer nets refuse it
    for flags, nl, hidden in ((capi.NGP_FF_SINGLE_WAVE, 2, 64), (capi.NGP_FF_LAYERED, 3, 64), (0, 4, 64), (0, 5, 64), (0, 2, 128)):
        assert _mlp_backward(lib, capi, flags, nl, hidden) == 1 and b'row bound' in lib.ngp_last_error(), (flags, nl, hidden)
    # the paired kernel's shapes pass that check (and stop at the next one: the tensors are NULL)
    for nl in (2, 3):
        assert _mlp_backward(lib, capi, 0, nl) == 1 and b'NULL tensor' in lib.ngp_last_error()
    # the grid backward: not with the grad_inputs kernel
    assert _grid_backward(lib, capi, ONE) == 1 and b'row bound' in lib.ngp_last_error()
    assert _grid_backward(lib, capi, None) == 1 and b'NULL tensor' in lib.ngp_last_error()
    # argument checks that come first stay first
    assert lib.ngp_ffmlp_backward_ex(None, None, None, None, 100, 32, 16, 64, 2, 0, 6, 1, None, None, None, capi.NGP_FF_SINGLE_WAVE, None) == 1
    assert b'128' in lib.ngp_last_error()


def test_null_disarms_and_the_entries_take_the_old_path(lib):
    import _ngp_capi as capi
    lib.ngp_training_row_bound(ONE)
    assert lib.ngp_training_row_bound(None) == 0
    for flags, nl, hidden in ((capi.NGP_FF_SINGLE_WAVE, 2, 64), (capi.NGP_FF_LAYERED, 3, 64), (0, 4, 64), (0, 2, 128)):
        assert _mlp_backward(lib, capi, flags, nl, hidden) == 1 and b'NULL tensor' in lib.ngp_last_error(), (flags, nl, hidden)
    assert _grid_backward(lib, capi, ONE) == 1 and b'NULL tensor' in lib.ngp_last_error()
    # `with capi.row_bound(None)` arms nothing; `with capi.row_bound(t)` disarms on the way out, also behind an exception

    class Word:
        def data_ptr(self):
            return 16
    with capi.row_bound(None):
        assert _mlp_backward(lib, capi, capi.NGP_FF_SINGLE_WAVE) == 1 and b'NULL tensor' in lib.ngp_last_error()
    with pytest.raises(ZeroDivisionError):
        with capi.row_bound(Word()):
            assert _mlp_backward(lib, capi, capi.NGP_FF_SINGLE_WAVE) == 1 and b'row bound' in lib.ngp_last_error()
            1 / 0
    assert _mlp_backward(lib, capi, capi.NGP_FF_SINGLE_WAVE) == 1 and b'NULL tensor' in lib.ngp_last_error()


def test_the_bound_belongs_to_the_thread_that_armed_it(lib):
    import _ngp_capi as capi
    lib.ngp_training_row_bound(ONE)
    seen = {}

    def other():
        seen['rc'] = _mlp_backward(lib, capi, capi.NGP_FF_SINGLE_WAVE)
        seen['msg'] = lib.ngp_last_error()
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen['rc'] == 1 and b'NULL tensor' in seen['msg']
    assert _mlp_backward(lib, capi, capi.NGP_FF_SINGLE_WAVE) == 1 and b'row bound' in lib.ngp_last_error()
