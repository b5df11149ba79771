"""CPU tests of the SVGP calls' workspace layout (csrc/gpx_svgp_layout.h): the four size functions return what they did
before the layout was written once (tests/golden/svgp_workspace_sizes.json, recorded by tools/svgp_workspace_sizes.py
from the library of the commit the file names), and the stand-alone host check of the layout itself passes."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from bayesianoptimizer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "svgp_workspace_sizes.json")


def test_reported_sizes_are_the_recorded_ones():
    lib = _capi.load()
    golden = json.load(open(GOLDEN))
    assert len(golden.pop("commit")) == 40
    assert sorted(golden) == ["gpx_svgp_bound_grad_workspace_size", "gpx_svgp_fit_collapsed_workspace_size",
                              "gpx_svgp_predict_workspace_size", "gpx_svgp_prepare_workspace_size"]
    # the whole grid (M 9 values, ntask 5, n 6, chunk 9, candidates 6): no case dropped
    assert [len(golden[f]) for f in sorted(golden)] == [9 * 6 * 5 * 9, 9 * 6 * 5 * 9, 9 * 6, 9 * 5]
    for rows in golden.values():
        assert len({tuple(r[:-1]) for r in rows}) == len(rows)  # and none twice
    bad = []
    for name, rows in golden.items():
        f = getattr(lib, name)
        for *args, want in rows:
            b = ctypes.c_size_t()
            st = f(*[ctypes.c_int64(a) for a in args], ctypes.byref(b))
            got = b.value if st == _capi.GPX_OK else -1
            if got != want:
                bad.append((name, args, want, got))
    assert not bad, bad[:10]


def test_layout_host_check(tmp_path):
    """tests/host/svgp_layout_check.cpp (includes the layout header alone) under the host compiler's address and
    undefined-behaviour sanitizers; without their runtimes on the machine it is built plain, and says so."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "host", "svgp_layout_check.cpp")
    exe = str(tmp_path / "svgp_layout_check")
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
    print("sanitizers:", "address,undefined" if sanitized else "none (runtimes not installed)")
