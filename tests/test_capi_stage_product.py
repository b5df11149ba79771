"""Host-side checks of gpx_debug_stage_product_f64 (no GPU): the symbol, its binding and the argument checks that need
no device.  The checks that need a live handle (row-tile range, shape, pitches) run in tests/test_gpu_sweep_narrow.py."""
import ctypes

import pytest

from bayesianoptimizer_amd import _capi

NEW = ["gpx_debug_stage_product_f64", "gpx_debug_stage_product_workspace_size"]


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def call(lib, h=None, n=384, W=None, ldw=384, K=None, ldk=128, ncols=32, lst=None, I0=0, nrows=1, shape=0, ss=None,
         ldss=128, ws=None, ws_bytes=0):
    return lib.gpx_debug_stage_product_f64(h, n, W, ldw, K, ldk, ncols, lst, I0, nrows, shape, ss, ldss, ws, ws_bytes)


def test_symbols_in_header_binding_and_library(lib):
    syms = _capi.header_symbols()
    for name in NEW:
        assert name in syms and name in _capi._PROTOS and hasattr(lib, name)


def test_invalid_arguments_are_rejected(lib):
    assert call(lib) == _capi.GPX_INVALID_ARG                       # null handle, null pointers
    assert call(lib, nrows=0) == _capi.GPX_INVALID_ARG
    assert call(lib, I0=2, nrows=2) == _capi.GPX_INVALID_ARG        # I0 + nrows > nI = 3
    assert call(lib, shape=2) == _capi.GPX_INVALID_ARG
    assert call(lib, shape=-1) == _capi.GPX_INVALID_ARG


def test_workspace_size(lib):
    b = ctypes.c_size_t()
    assert lib.gpx_debug_stage_product_workspace_size(300, None) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_stage_product_workspace_size(0, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_stage_product_workspace_size(300, ctypes.byref(b)) == _capi.GPX_OK
    assert 384 * 8 <= b.value < 1 << 16  # an {output column, slot} pair per slot of the three 128-column tiles
