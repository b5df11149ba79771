"""CPU tests of the pruned top-k sweep's host side: gpx_acquire_topk_workspace_size, and ExactGP.sweep_objective_topk /
the drop-in's analytic sweep through tests/oracle_engine.py, which has no acquire_topk and so takes the composition
(full sweep with scores + topk)."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, _capi
from bayesianoptimizer_amd.models import ExactGP
from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
from oracle import gp_oracle as O
from tests.oracle_engine import OracleEngine
from tests.stubs import BOUNDS, StubSimulator


def _size(lib, n, m, k):
    b = ctypes.c_size_t()
    st = lib.gpx_acquire_topk_workspace_size(n, m, k, ctypes.byref(b))
    return st, b.value


def _up256(b):
    return (b + 255) // 256 * 256


def _chunk(npad, m):
    cap = min(max(((1 << 30) // 8 // npad) // 256 * 256, 256), 1 << 20)
    return min(max(_up256(m), 256), cap)


def test_workspace_size_is_the_sweep_workspace_plus_the_documented_topk_part():
    lib = _capi.load()
    assert _capi.GPX_TOPK_SWEEP_MAX == 1024
    assert "GPX_TOPK_SWEEP_MAX = 1024" in open(_capi.HEADER_PATH).read()
    for n, m, k in [(300, 5000, 16), (640, 5000, 1024), (4096, 1 << 20, 64), (1000, 700, 700), (100, 10, 1)]:
        st, total = _size(lib, n, m, k)
        assert st == _capi.GPX_OK
        sweep, sort = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.gpx_sweep_workspace_size(n, 1, m, ctypes.byref(sweep)) == _capi.GPX_OK
        assert lib.gpx_topk_workspace_size(m, ctypes.byref(sort)) == _capi.GPX_OK
        C = _chunk(lib.gpx_padded_n(n), m)
        # header + alignment slack, pool (k pairs), scored list (a pair per candidate of a chunk), the composed path's
        # scores and its sort workspace
        part = 512 + 2 * _up256(8 * k) + 2 * _up256(8 * C) + _up256(8 * m) + sort.value
        assert total == sweep.value + part, (n, m, k)


def test_workspace_size_grows_with_k_and_m_and_rejects_bad_k():
    lib = _capi.load()
    sizes_k = [_size(lib, 640, 5000, k)[1] for k in (1, 64, 300, 1024)]
    assert sizes_k == sorted(sizes_k) and len(set(sizes_k)) == 4
    sizes_m = [_size(lib, 640, m, 16)[1] for m in (1000, 5000, 100_000)]
    assert sizes_m == sorted(sizes_m) and len(set(sizes_m)) == 3
    for n, m, k in [(640, 5000, 0), (640, 5000, 1025), (640, 700, 701), (640, 5000, -3), (0, 5000, 4), (640, 0, 1)]:
        assert _size(lib, n, m, k)[0] == _capi.GPX_INVALID_ARG, (n, m, k)
    assert lib.gpx_acquire_topk_workspace_size(640, 5000, 16, None) == _capi.GPX_INVALID_ARG
    # the sweep's own size is what it was (tests/test_capi_sweep_lazy.py pins the bytes)
    assert lib.gpx_acquire_topk_f64(None, None, 1, None, 1, None, 1, None, None, 1, 1, None, 0, 1, None, None, None,
                                    0) == _capi.GPX_INVALID_ARG


@pytest.mark.parametrize("shared", [True, False])
def test_sweep_objective_topk_composes_on_an_engine_without_acquire_topk(shared):
    eng = OracleEngine()
    assert not hasattr(eng, "acquire_topk")
    n, d, T, m, k = 40, 3, 3, 200, 7
    rng = np.random.default_rng(3)
    X = rng.random((n, d))
    Y = np.stack([np.sin((3 + q) * X).sum(1) for q in range(T)], 1)
    kp = KernelParams("matern52", 0.6, noise=1e-4)
    gp = ExactGP(torch.tensor(X), torch.tensor(Y), kp if shared else [kp] * T, engine=eng).fit()
    assert gp.independent == (not shared)
    Xs = torch.tensor(O.sobol_candidates(m, d, 5))
    w = [0.5, 1.0, 0.25]
    _, _, scores = gp.sweep_objective(Xs, "ucb", w, beta=4.0, return_scores=True)
    before = dict(eng.calls)
    val, idx = gp.sweep_objective_topk(Xs, "ucb", w, k, beta=4.0, index_offset=1000)
    v_ref, i_ref = O.topk_desc(scores.numpy(), k)
    assert idx.tolist() == [1000 + int(i) for i in i_ref]
    assert np.array_equal(val.numpy(), v_ref)
    key = "acquire" if shared else "acquire_multi"
    assert eng.calls[key] == before.get(key, 0) + 1 and eng.calls["topk"] == before.get("topk", 0) + 1


def test_dropin_analytic_sweep_goes_through_sweep_objective_topk(tmp_path, monkeypatch):
    eng = OracleEngine()
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=30, n_batches=0, batch_size=4,
                            target_total=30, engine=eng, seed=5,
                            gp_config=GPConfig(fit_hyperparameters=False, raw_samples=256), acquisition="logei")
    opt.optimize()
    opt.fit_gp_model()
    grid = opt._sobol_grid(256)
    monkeypatch.setattr(opt, "_sobol_grid", lambda n: grid[:n])
    got = opt._analytic_sweep(5)
    gp, w = opt.gp_model, opt._acq_weights()
    gt = opt._tensor(grid)
    _, _, score = gp.sweep_objective(opt.x_tf(gt), "logei", w.tolist(), best_f=opt._incumbent(w),
                                     beta=opt.config.beta, return_scores=True)
    _, order = eng.topk(score, 5)
    assert torch.equal(got, gt[order])
