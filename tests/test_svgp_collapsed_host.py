"""Closed-form SVGP variational posterior, host side (no GPU): the NumPy restatement (tests/sgpr_ref.py) is the optimum
of the ELBO it claims to be, the C ABI's host-only parts answer, and select_inducing_points mirrors
optimization/Bayesian7.py:109-123."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from bayesianoptimizer_amd.svgp import select_inducing_points
from oracle import gp_oracle as O
from tests import sgpr_ref as R


@pytest.fixture(scope="module")
def task3():
    pb = R.problem(3)
    return pb, R.fit_collapsed_task(pb.Z[0], pb.X, pb.Y[:, 0], pb.ops[0])


def elbo(Phi, r, s2, kdiag_sum, m, S):
    """The uncollapsed whitened ELBO at q(u) = N(m, S): E_q[log N(y | c + Phi^T u, s2 I)] - (1/2 s2) tr(K_ff - Q_ff)
    - KL(N(m, S) || N(0, I)), f's conditional variance given u being K_ff - Phi^T Phi."""
    n, M = r.shape[0], m.shape[0]
    resid = r - Phi.T @ m
    ell = (-0.5 * n * np.log(2.0 * np.pi * s2) - 0.5 * (resid @ resid) / s2
           - 0.5 * np.einsum("ij,ij->", Phi, S @ Phi) / s2
           - 0.5 * (kdiag_sum - np.einsum("ij,ij->", Phi, Phi)) / s2)
    _, logdet_s = np.linalg.slogdet(S)
    kl = 0.5 * (np.trace(S) + m @ m - M - logdet_s)
    return ell - kl


def test_reference_is_the_stationary_point(task3):
    _, f = task3
    B, b, m, S, C = f["B"], f["b"], f["m"], f["S"], f["C"]
    assert np.abs(B @ m - b).max() <= 1e-10 * np.abs(b).max()
    assert np.abs(B @ S - np.eye(B.shape[0])).max() <= 1e-10
    assert np.abs(C @ C.T - S).max() <= 1e-10 * np.abs(S).max()
    assert np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)


def test_full_elbo_at_the_optimum_equals_the_collapsed_bound(task3):
    pb, f = task3
    p = pb.ops[0]
    kd = O.kernel_diag(pb.X, p).sum()
    full = elbo(f["Phi"], f["r"], p.noise, kd, f["m"], f["S"])
    scale = np.abs(f["terms"]).sum()
    assert abs(full - f["F"]) <= 1e-9 * scale
    assert f["F"] == pytest.approx(f["terms"].sum(), rel=1e-15)


def test_elbo_is_lower_away_from_the_optimum(task3):
    pb, f = task3
    p = pb.ops[0]
    kd = O.kernel_diag(pb.X, p).sum()
    best = elbo(f["Phi"], f["r"], p.noise, kd, f["m"], f["S"])
    rng = np.random.default_rng(5)
    for _ in range(3):
        delta = 1e-2 * rng.standard_normal(f["m"].shape[0])
        assert elbo(f["Phi"], f["r"], p.noise, kd, f["m"] + delta, f["S"]) < best


def test_bound_is_below_the_exact_evidence():
    pb = R.problem(1)
    f = R.fit_collapsed_task(pb.Z[0], pb.X, pb.Y[:, 0], pb.ops[0])
    exact = -O.mll_value_grad(pb.X, pb.Y[:, 0], pb.ops[0])["nll"]
    print(f"collapsed bound {f['F']:.4f} <= exact log evidence {exact:.4f}")
    assert np.isfinite(f["F"]) and f["F"] <= exact


# ---- the C ABI's host-only parts ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def test_symbols_exported_and_bound_layout_matches_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (gpx_[a-z0-9_]+)\b", out))
    assert {"gpx_svgp_fit_collapsed_workspace_size", "gpx_svgp_fit_collapsed_f64"} <= exported
    hdr = open(_capi.HEADER_PATH).read()
    for name in ("F", "CONST", "LOGDET", "QUAD", "FIT", "TRACE", "NOUT"):
        assert re.search(rf"\bGPX_SVGP_BOUND_{name} = {getattr(_capi, 'SVGP_BOUND_' + name)}\b", hdr), name
    assert re.search(rf"#define GPX_SVGP_FIT_CHUNK {_capi.SVGP_FIT_CHUNK}\b", hdr)


def test_workspace_query_without_gpu(lib):
    def size(M, n, T, chunk):
        b = ctypes.c_size_t()
        assert lib.gpx_svgp_fit_collapsed_workspace_size(M, n, T, chunk, ctypes.byref(b)) == _capi.GPX_OK
        return b.value

    M, T = 2048, 8
    # grows with the chunk width; at least W and B per task and the two M x chunk buffers
    s128, s1024, sdef = size(M, 100000, T, 128), size(M, 100000, T, 1024), size(M, 100000, T, 0)
    assert s128 < s1024 < sdef
    assert sdef == size(M, 100000, T, _capi.SVGP_FIT_CHUNK)
    assert s1024 >= T * 2 * M * M * 8 + 2 * M * 1024 * 8
    assert size(M, 100000, T, 1000) == s1024  # rounded up to a multiple of 128
    # bounded independently of n: the same beyond one chunk, and far below the exact factor's 2 n^2 doubles
    assert sdef == size(M, 10 ** 6, T, 0) == size(M, 10 ** 7, T, 0)
    assert sdef < 2 * 10 ** 9
    assert size(M, 300, T, 0) <= sdef
    b = ctypes.c_size_t()
    for bad in ((0, 10, 1, 0), (10, 0, 1, 0), (10, 10, 0, 0), (10, 10, 1, -1)):
        assert lib.gpx_svgp_fit_collapsed_workspace_size(*bad, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_svgp_fit_collapsed_workspace_size(10, 10, 1, 0, None) == _capi.GPX_INVALID_ARG


def test_null_handle_is_rejected(lib):
    # (null pointers behind a live handle: tests/test_gpu_svgp_collapsed.py, a handle needs a device)
    p = (_capi.KernelParamsC * 1)()
    one = ctypes.c_void_p(256)  # never dereferenced: the call is refused first
    args = [p, 1, 4, 1e-4, one, 3, 12, one, 10, 3, one, 1, one, 4, one, 4, 16, one, one, one, 1 << 20]
    assert lib.gpx_svgp_fit_collapsed_f64(None, *args) == _capi.GPX_INVALID_ARG


def test_python_bound_indices_are_the_terms_in_order():
    assert [_capi.SVGP_BOUND_F, _capi.SVGP_BOUND_CONST, _capi.SVGP_BOUND_LOGDET, _capi.SVGP_BOUND_QUAD,
            _capi.SVGP_BOUND_FIT, _capi.SVGP_BOUND_TRACE, _capi.SVGP_BOUND_NOUT] == list(range(7))


# ---- select_inducing_points -----------------------------------------------------------------------------------
class _CpuFps:
    def __init__(self):
        self.calls = []

    def fps(self, X, k, start):
        self.calls.append((tuple(X.shape), int(k), int(start)))
        return R.fps_cpu(X.numpy(), k, start)


def test_select_inducing_points_sizes_and_subsampling():
    X = torch.tensor(np.random.default_rng(0).random((300, 4)))
    eng = _CpuFps()
    # fewer rows than the subset: FPS over all of them, m distinct rows of X, from a start inside the range
    Z = select_inducing_points(X, 16, subset_size=1000, generator=torch.Generator().manual_seed(1), engine=eng)
    assert Z.shape == (16, 4) and eng.calls[-1][:2] == ((300, 4), 16) and 0 <= eng.calls[-1][2] < 300
    rows = {tuple(r) for r in X.numpy().tolist()}
    assert len({tuple(r) for r in Z.numpy().tolist()}) == 16 and all(tuple(r) in rows for r in Z.numpy().tolist())
    # more rows than the subset: a random subsample of subset_size rows first
    Z = select_inducing_points(X, 16, subset_size=50, generator=torch.Generator().manual_seed(1), engine=eng)
    assert Z.shape == (16, 4) and eng.calls[-1][:2] == ((50, 4), 16) and 0 <= eng.calls[-1][2] < 50
    assert all(tuple(r) in rows for r in Z.numpy().tolist())
    # m at least the rows kept: all of them, without FPS (farthest_point_sampling returns its input, :88-89)
    ncalls = len(eng.calls)
    Z = select_inducing_points(X, 64, subset_size=50, generator=torch.Generator().manual_seed(2), engine=eng)
    assert Z.shape == (50, 4) and len(eng.calls) == ncalls
    assert select_inducing_points(X[:10], 64, engine=eng).shape == (10, 4)
    # the same generator state gives the same points
    a = select_inducing_points(X, 16, subset_size=50, generator=torch.Generator().manual_seed(7), engine=eng)
    b = select_inducing_points(X, 16, subset_size=50, generator=torch.Generator().manual_seed(7), engine=eng)
    assert torch.equal(a, b)
