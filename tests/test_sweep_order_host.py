"""CPU tests of the mean-first order's C ABI additions: libgpx.so exports the sweep_order switch and the
list-driven head's debug entry, _capi.py binds them with the header's argument counts, the switch rejects a null handle
without a GPU, and the workspace the order runs in is the size the parent build reported (it adds no region)."""
import ctypes
import re

import pytest

from bayesianoptimizer_amd import _capi

NEW = ["gpx_debug_set_sweep_order", "gpx_debug_get_sweep_order", "gpx_debug_head_product_list_f64"]


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


@pytest.mark.parametrize("name", NEW)
def test_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name)
    assert name in _capi.header_symbols()
    restype, argtypes = _capi._PROTOS[name]
    assert restype is ctypes.c_int32
    with open(_capi.HEADER_PATH) as f:
        decl = re.search(rf"gpx_status {name}\((.*?)\);", f.read(), re.S).group(1)
    assert len(argtypes) == decl.count(",") + 1


def test_list_entry_is_the_contiguous_entry_plus_list_and_count():
    base = _capi._PROTOS["gpx_debug_head_product_f64"][1]
    assert _capi._PROTOS["gpx_debug_head_product_list_f64"][1][:len(base)] == base
    assert len(_capi._PROTOS["gpx_debug_head_product_list_f64"][1]) == len(base) + 2


def test_null_handle_is_rejected(lib):
    v = ctypes.c_int32(7)
    assert lib.gpx_debug_set_sweep_order(None, 1) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_get_sweep_order(None, ctypes.byref(v)) == _capi.GPX_INVALID_ARG
    assert v.value == 7


def test_workspace_sizes_are_the_parents(lib):
    # gpx_sweep_workspace_size(n, 1, m) of the parent build (commit aa478a3), read through its library
    for (n, m), want in {(4096, 1 << 20): 3792374096, (384, 400_000): 2351392832, (640, 250_000): 2195630880}.items():
        b = ctypes.c_size_t()
        assert lib.gpx_sweep_workspace_size(n, 1, m, ctypes.byref(b)) == _capi.GPX_OK
        assert b.value == want
