"""Host-side checks of the mean bound's ABI additions (no GPU): the debug entry points and the unchanged workspace."""
import ctypes

import pytest

from bayesianoptimizer_amd import _capi

NEW = ["gpx_debug_mu_bound_f64", "gpx_debug_mu_bound_workspace_size", "gpx_debug_kstar_mu_f64"]
# gpx_sweep_workspace_size(n, 1, m) of the library before the mean bound: its hand-off values live in arrays the sweep had
WORKSPACE_BEFORE = {(4096, 1 << 20): 3792374096, (16384, 1 << 22): 3787643216, (100096, 1 << 22): 3745005840,
                    (384, 5000): 33631504}


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def test_symbols_in_header_binding_and_library(lib):
    syms = _capi.header_symbols()
    for name in NEW:
        assert name in syms and name in _capi._PROTOS and hasattr(lib, name)


def test_null_arguments_are_rejected(lib):
    assert lib.gpx_debug_mu_bound_f64(None, None, 300, None, 4, None, None, 10, 4, None, None, None, 0) == \
        _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_kstar_mu_f64(None, None, 300, None, 4, None, None, 10, 4, None, None, None, 256, None, 256) == \
        _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_mu_bound_workspace_size(300, None) == _capi.GPX_INVALID_ARG
    b = ctypes.c_size_t()
    assert lib.gpx_debug_mu_bound_workspace_size(0, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_mu_bound_workspace_size(300, ctypes.byref(b)) == _capi.GPX_OK
    assert 0 < b.value < 1 << 20


@pytest.mark.parametrize("n,m", sorted(WORKSPACE_BEFORE))
def test_sweep_workspace_did_not_grow(lib, n, m):
    b = ctypes.c_size_t()
    assert lib.gpx_sweep_workspace_size(n, 1, m, ctypes.byref(b)) == _capi.GPX_OK
    assert b.value == WORKSPACE_BEFORE[(n, m)]
