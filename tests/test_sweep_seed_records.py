"""CPU test of the records the lazy pruned sweep writes with its first span seeded from the head bound: the
stand-alone host check tests/host/sweep_seed_records_check.cpp, a second statement of the spans, the seed round and the
rounds against csrc/gpx_sweep_layout.h, passes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_records_host_check(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers; without their runtimes on the machine
    it is built plain, and says so."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "host", "sweep_seed_records_check.cpp")
    exe = str(tmp_path / "sweep_seed_records_check")
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
    assert "record plans checked, 0 failures" in run.stdout
    print("sanitizers:", "address,undefined" if sanitized else "none (runtimes not installed)")
