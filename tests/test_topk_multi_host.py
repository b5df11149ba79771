"""CPU tests of the pruned multi-output top-k sweep's host side (gpx_acquire_topk_multi_f64): the size function, the
entry point's NULL-handle check, the routing of ExactGP.sweep_objective_topk on a stub engine, the stand-alone check of
the workspace layout, and the oracle's replay of the bound on the test problem of tests/multi_sweep_util.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, _capi
from bayesianoptimizer_amd.models import ExactGP
from oracle import gp_oracle as O
from tests import multi_sweep_util as U
from tests.oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _size(lib, n, m, k):
    b = ctypes.c_size_t()
    st = lib.gpx_acquire_topk_multi_workspace_size(n, m, k, ctypes.byref(b))
    return st, b.value


def test_workspace_size_grows_with_k_and_m_and_rejects_bad_arguments():
    lib = _capi.load()
    sizes_k = [_size(lib, 640, 5000, k)[1] for k in (1, 64, 300, 1024)]
    assert sizes_k == sorted(sizes_k) and len(set(sizes_k)) == 4
    sizes_m = [_size(lib, 640, m, 16)[1] for m in (1000, 5000, 100_000)]
    assert sizes_m == sorted(sizes_m) and len(set(sizes_m)) == 3
    for n, m, k in [(640, 5000, 0), (640, 5000, -3), (640, 5000, 1025), (640, 700, 701), (0, 5000, 4), (640, 0, 1)]:
        assert _size(lib, n, m, k)[0] == _capi.GPX_INVALID_ARG, (n, m, k)
    assert lib.gpx_acquire_topk_multi_workspace_size(640, 5000, 16, None) == _capi.GPX_INVALID_ARG
    for n, m, k in [(300, 5000, 16), (640, 5000, 1024), (4096, 1 << 20, 64), (1000, 700, 700), (100, 10, 1)]:
        st, total = _size(lib, n, m, k)
        multi, sort = ctypes.c_size_t(), ctypes.c_size_t()
        assert st == _capi.GPX_OK
        assert lib.gpx_sweep_multi_workspace_size(n, m, ctypes.byref(multi)) == _capi.GPX_OK
        assert lib.gpx_topk_workspace_size(m, ctypes.byref(sort)) == _capi.GPX_OK
        # at least the multi-output sweep's, plus the pool, the composed path's scores and its sort workspace
        assert total >= multi.value + 16 * k + 8 * m + sort.value, (n, m, k)


def test_entry_point_rejects_a_null_handle():
    lib = _capi.load()
    assert lib.gpx_acquire_topk_multi_f64(None, None, 1, 1, None, 1, None, None, None, None, None, None, None, 1, 1,
                                          None, 0, 1, None, None, None, 0) == _capi.GPX_INVALID_ARG


class StubEngine(OracleEngine):
    """OracleEngine with the multi-output top-k call: the composition, counted."""

    def acquire_topk_multi(self, states, Xs, k, kind="logei", best_f=0.0, beta=4.0, weights=None, y_mean=None,
                           y_scale=None, index_offset=0):
        self.calls["acquire_topk_multi"] = self.calls.get("acquire_topk_multi", 0) + 1
        _, _, scores = OracleEngine.acquire_multi(self, states, Xs, kind, best_f, beta, weights, y_mean, y_scale,
                                                  return_scores=True)
        v, i = O.topk_desc(scores.numpy(), int(k))
        return torch.tensor(v), torch.tensor(i + index_offset)


@pytest.mark.parametrize("shared", [False, True])
def test_sweep_objective_topk_routing(shared):
    eng = StubEngine()
    n, d, T, m, k = 40, 3, 3, 1100, 7
    rng = np.random.default_rng(3)
    X = rng.random((n, d))
    Y = np.stack([np.sin((3 + q) * X).sum(1) for q in range(T)], 1)
    kp = KernelParams("matern52", 0.6, noise=1e-4)
    gp = ExactGP(torch.tensor(X), torch.tensor(Y), kp if shared else [kp] * T, engine=eng).fit()
    assert gp.independent == (not shared)
    Xs = torch.tensor(O.sobol_candidates(m, d, 5))
    w = [0.5, 1.0, 0.25]
    _, _, scores = gp.sweep_objective(Xs, "ucb", w, beta=4.0, return_scores=True)
    v_ref, i_ref = O.topk_desc(scores.numpy(), k)
    val, idx = gp.sweep_objective_topk(Xs, "ucb", w, k, beta=4.0, index_offset=1000)
    assert idx.tolist() == [1000 + int(i) for i in i_ref] and np.array_equal(val.numpy(), v_ref)
    assert eng.calls.get("acquire_topk_multi", 0) == (0 if shared else 1)
    # k beyond the pool composes the full sweep and topk
    before = dict(eng.calls)
    val, idx = gp.sweep_objective_topk(Xs, "ucb", w, 1025, beta=4.0)
    v_ref, i_ref = O.topk_desc(scores.numpy(), 1025)
    assert idx.tolist() == [int(i) for i in i_ref] and np.array_equal(val.numpy(), v_ref)
    assert eng.calls.get("acquire_topk_multi", 0) == before.get("acquire_topk_multi", 0)
    assert eng.calls["topk"] == before.get("topk", 0) + 1


def test_layout_host_check(tmp_path):
    """tests/host/topk_multi_layout_check.cpp (includes the layout header alone) under the host compiler's address and
    undefined-behaviour sanitizers; without their runtimes on the machine it is built plain, and says so."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "host", "topk_multi_layout_check.cpp")
    exe = str(tmp_path / "topk_multi_layout_check")
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


@pytest.mark.parametrize("n", [384, 640, 1000])
@pytest.mark.parametrize("acq", ["ei", "logei", "ucb"])
def test_oracle_replay_of_the_bound_prunes(n, acq):
    """T = 3, k = 16: the seed block and the staged candidates whose bound (the variance of the first 128 rows of every
    output's L^-1 K*, per-output floors) reaches the 16th best seed score are at most half of the candidates."""
    surv = U.oracle_survivors(n, acq, 16)
    print(f"n = {n}, {acq}: {surv} of {U.M - U.SEED_BLOCK} staged candidates survive")
    assert U.SEED_BLOCK + surv <= U.M / 2
