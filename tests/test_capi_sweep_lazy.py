"""Host-side checks of the lazy pruned sweep's ABI additions (no GPU): the workspace cap and gpx_debug_kstar_f64."""
import ctypes

import pytest

from bayesianoptimizer_amd import _capi

GIB = 1 << 30


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def ws_bytes(lib, n, m):
    b = ctypes.c_size_t()
    assert lib.gpx_sweep_workspace_size(n, 1, m, ctypes.byref(b)) == _capi.GPX_OK
    return b.value


def chunked_pruned_bytes(npad, m):
    """gpx_sweep_workspace_size of the chunked pruned sweep (the size before the head phase's arrays were added)."""
    cap = max(256, min(1 << 20, (GIB // 8 // npad) // 256 * 256))
    C = min(max(256, (m + 255) // 256 * 256), cap)
    up = lambda v: (v + 127) // 128 * 128
    full = npad * C * 8 + (npad // 64) * C * 8 + (npad // 128) * C * 8 + ((m + 255) // 256 + 1) * 16 + 256
    return full + 1024 + 2 * C * 8 + npad * (up(C // 2) + up(C // 4)) * 8


def test_workspace_cap_at_the_bench_shape(lib):
    """Head rows, mean and variance partials of 2^20 candidates (1.75 GiB) on top of the chunked sweep's 1.77 GiB."""
    new, old = ws_bytes(lib, 4096, 1 << 20), chunked_pruned_bytes(4096, 1 << 20)
    print(f"workspace at (4096, 1, 2^20): {new} bytes = {new / GIB:.3f} GiB, {new / old:.3f} x the chunked sweep's")
    assert old + 1.75 * GIB <= new < 2.25 * old


@pytest.mark.parametrize("n", [16384, 100096])
def test_byte_budget_bounds_the_head_phase_at_large_n(lib, n):
    new, old = ws_bytes(lib, n, 1 << 22), chunked_pruned_bytes(n, 1 << 22)
    print(f"workspace at ({n}, 1, 2^22): {new} bytes = {new / GIB:.3f} GiB; head phase {(new - old) / GIB:.3f} GiB")
    # 1.75 GiB of per-candidate arrays, the survivor list (8 bytes per candidate) and the records
    assert new - old <= 1.75 * GIB + (1 << 20) * 8 + (1 << 22) // 256 * 2 * 16 + 4096


def test_small_calls_pay_for_their_own_size_only(lib):
    assert ws_bytes(lib, 384, 5000) < 4 * chunked_pruned_bytes(384, 5000)
    assert ws_bytes(lib, 256, 1 << 12) < 2 * 256 * 4096 * 8  # the fused sizes carry no pruned-sweep arrays


def test_debug_kstar_symbol_in_header_and_binding(lib):
    syms = _capi.header_symbols()
    assert "gpx_debug_kstar_f64" in syms and "gpx_debug_kstar_workspace_size" in syms
    assert "gpx_debug_kstar_f64" in _capi._PROTOS
    assert hasattr(lib, "gpx_debug_kstar_f64")
    b = ctypes.c_size_t()
    assert lib.gpx_debug_kstar_workspace_size(300, 3072, ctypes.byref(b)) == _capi.GPX_OK
    assert b.value >= (384 // 64) * 3072 * 8
    assert lib.gpx_debug_kstar_f64(None, None, 300, None, 4, None, 10, 4, None, None, None, 256, None, 0) == \
        _capi.GPX_INVALID_ARG
