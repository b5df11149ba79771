"""CPU tests of the pruned sweep's tail read-back: the stand-alone host check of sweep_tail_rounds
(tests/host/sweep_tail_rounds_check.cpp against csrc/gpx_sweep_layout.h) passes, libgpx.so exports the sweep_tail_sync
switch and the rounds getter, _capi.py binds them with the header's argument counts, and they reject a null handle
without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from bayesianoptimizer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpx_debug_set_sweep_tail_sync", "gpx_debug_get_sweep_tail_sync", "gpx_debug_get_tail_rounds"]


def test_tail_rounds_host_check(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers; without their runtimes on the machine
    it is built plain, and says so."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "host", "sweep_tail_rounds_check.cpp")
    exe = str(tmp_path / "sweep_tail_rounds_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    built = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                           text=True)
    sanitized = built.returncode == 0
    if not sanitized:
        print("sanitizer build failed, building without:\n" + built.stderr[-2000:])
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0
    assert "tail round checks, 0 failures" in run.stdout
    print("sanitizers:", "address,undefined" if sanitized else "none (runtimes not installed)")


@pytest.mark.parametrize("name", NEW)
def test_exported_declared_and_bound(name):
    lib = _capi.load()
    assert hasattr(lib, name)
    assert name in _capi.header_symbols()
    restype, argtypes = _capi._PROTOS[name]
    assert restype is ctypes.c_int32
    with open(_capi.HEADER_PATH) as f:
        decl = re.search(rf"gpx_status {name}\((.*?)\);", f.read(), re.S).group(1)
    assert len(argtypes) == decl.count(",") + 1


def test_null_handle_is_rejected():
    lib = _capi.load()
    v = ctypes.c_int32(7)
    out = (ctypes.c_int64 * 3)(5, 6, 7)
    assert lib.gpx_debug_set_sweep_tail_sync(None, 1) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_get_sweep_tail_sync(None, ctypes.byref(v)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_debug_get_tail_rounds(None, out) == _capi.GPX_INVALID_ARG
    assert v.value == 7 and list(out) == [5, 6, 7]
