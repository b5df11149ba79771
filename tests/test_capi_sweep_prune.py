"""Host-side checks of the pruned sweep's ABI additions (no GPU): option slot 8 and gpx_sweep_stats."""
import ctypes
import os
import re

import pytest

from bayesianoptimizer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def test_option_slot_in_header_and_binding():
    hdr = open(_capi.HEADER_PATH).read()
    assert _capi.OPTIONS["sweep_prune"] == 8
    assert re.search(r"\bGPX_OPT_SWEEP_PRUNE = 8\b", hdr)
    assert _capi.GPX_OPT_COUNT == 9 and re.search(r"\bGPX_OPT_COUNT = 9\b", hdr)
    # earlier slots keep their numbers
    assert _capi.OPTIONS["sweep_fused"] == 2 and _capi.OPTIONS["potrf_split"] == 7


def test_option_name_is_in_the_env_parser_table():
    """GPX_OPTIONS names are matched against one table in gpx_capi.cpp, indexed by option number (parsing itself needs a
    handle, hence a device: tests/test_gpu_sweep_prune.py::test_env_option_parses)."""
    src = open(os.path.join(ROOT, "bayesianoptimizer_amd", "csrc", "gpx_capi.cpp")).read()
    table = re.search(r"names\[GPX_OPT_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r'"([a-z_]*)"', table)
    assert names.index("sweep_prune") == 8 and len(names) == _capi.GPX_OPT_COUNT
    for name, slot in _capi.OPTIONS.items():
        assert names[slot] == name


def test_sweep_stats_symbol_and_null_handle(lib):
    assert "gpx_sweep_stats" in _capi.header_symbols()
    out = (ctypes.c_int64 * 4)()
    assert lib.gpx_sweep_stats(None, out) == _capi.GPX_INVALID_ARG


def test_workspace_covers_the_compact_buffers(lib):
    """One K* chunk plus the two compact buffers of a half and a quarter of it (single output, padded n >= 384)."""
    b = ctypes.c_size_t()
    assert lib.gpx_sweep_workspace_size(4096, 1, 1 << 20, ctypes.byref(b)) == _capi.GPX_OK
    chunk = 4096 * 32768 * 8
    assert b.value >= chunk + chunk // 2 + chunk // 4
    small = ctypes.c_size_t()
    assert lib.gpx_sweep_workspace_size(256, 1, 1 << 12, ctypes.byref(small)) == _capi.GPX_OK
    assert small.value < 2 * 256 * 4096 * 8  # the fused sizes carry no compact buffers
