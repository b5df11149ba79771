"""CPU tests of the workspace of gpx_svgp_bound_grad_z_f64 (the kind SVGP_GRAD_Z of csrc/gpx_svgp_layout.h): the
stand-alone host check of the layout passes, and the three pinned sizes (tests/golden/svgp_z_workspace_sizes.json:
the gradient's recorded size plus ntask Mpad 32 8 bytes of accumulators plus (Mpad / 128) max(Mpad / 128, C / 128) 128 32
8 bytes of row partials, each rounded up to 256) are what the layout header and the library's size function report."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from bayesianoptimizer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "svgp_z_workspace_sizes.json")
CASES = [(130, 1, 128), (200, 3, 256), (2048, 8, 4096)]


def golden_sizes():
    rows = json.load(open(GOLDEN))["gpx_svgp_bound_grad_z_workspace_size"]
    assert [tuple(r[:3]) for r in rows] == CASES
    return {tuple(r[:3]): r[3] for r in rows}


def test_layout_host_check(tmp_path):
    """tests/host/svgp_layout_z_check.cpp under the host compiler's address and undefined-behaviour sanitizers; without
    their runtimes on the machine it is built plain, and says so."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "host", "svgp_layout_z_check.cpp")
    exe = str(tmp_path / "svgp_layout_z_check")
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
    assert "layouts checked, 0 failures" in run.stdout
    sizes = {tuple(int(v) for v in line.split()[1:4]): int(line.split()[4])
             for line in run.stdout.splitlines() if line.startswith("size ")}
    assert sizes == golden_sizes()
    print("sanitizers:", "address,undefined" if sanitized else "none (runtimes not installed)")


def test_size_function_reports_the_pinned_sizes():
    lib = _capi.load()
    want = golden_sizes()
    for (M, T, chunk), size in want.items():
        for n in (700, 100_000):  # the size does not depend on n
            b = ctypes.c_size_t()
            assert lib.gpx_svgp_bound_grad_z_workspace_size(M, n, T, chunk, ctypes.byref(b)) == _capi.GPX_OK
            assert b.value == size, (M, T, chunk, n)
        g = ctypes.c_size_t()
        assert lib.gpx_svgp_bound_grad_workspace_size(M, 700, T, chunk, ctypes.byref(g)) == _capi.GPX_OK
        Mpad = (M + 127) // 128 * 128
        up = lambda v: (v + 255) // 256 * 256  # noqa: E731
        assert size == g.value + T * up(Mpad * 32 * 8) + up((Mpad // 128) * max(Mpad // 128, chunk // 128) * 128 * 32 * 8)
    b = ctypes.c_size_t()
    assert lib.gpx_svgp_bound_grad_z_workspace_size(0, 700, 1, 128, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_svgp_bound_grad_z_workspace_size(130, 700, 1, 128, None) == _capi.GPX_INVALID_ARG
