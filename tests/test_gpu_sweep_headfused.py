"""The fused head of the lazy pruned sweep (head_product_kernel) against the two launches it replaces.

Yardstick: bit identity.  (1) gpx_debug_head_product_f64 runs the production kernel; its reference is the composition
gpx_debug_kstar_mu_f64 (full build) followed by gpx_debug_stage_product_f64 (row tile 0, the wide shape) on that build's
rows 0 .. 127: ss and the mean partials of row blocks 0 and 1 are compared as int64 patterns, NaNs at the same places.
n = 40 (row block 1 all padding), 100 (partly padding), 300; d = 3 / 8 / 16 (every DMAX); the three kernel kinds with
per-dimension lengthscales; m = 1000 and 129 (partial last column groups of 128 and of 256).  The candidates hold copies
of training rows, a far block, one NaN row and one infinite coordinate.  W is the fit's own L^-T at n = 300, else a
random upper-triangular matrix.  (2) acquire and acquire_topk at n = 640 under sweep_head = 1 and 0: values, indices and
sweep_stats.  sweep_prune = 2 puts n = 640 on the pruned path whatever the default threshold; the staged path is asserted
to have run."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ["rbf", "matern52", "scale_linear_matern52"]
_cases = {}
_fits = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def ptr(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


def bits(a):
    return a.contiguous().view(torch.int64)


def params(kind, d):
    rng = np.random.default_rng(100 + d)
    ls = botorch_default_lengthscale(d) * rng.uniform(0.6, 1.6, d)
    lv = rng.uniform(0.2, 1.5, d)
    return KernelParams(kind, [float(v) for v in ls], outputscale=1.3, noise=1e-4,
                        linear_variance=[float(v) for v in lv])


def candidates(X, m, rng):
    n, d = X.shape
    Xs = rng.random((m, d))
    q = m // 8
    Xs[q:2 * q] = X[rng.integers(0, n, q)]   # copies of training rows
    Xs[2 * q:3 * q] *= 50.0                   # a far block
    Xs[3 * q + 5] = np.nan                    # one NaN row
    Xs[m - 3, d - 1] = np.inf                 # one infinite coordinate, in the partial last group
    return Xs


def case(engine, kind, n, d):
    """(kernel parameters, X, alpha, W) of one model, shared by the module and never modified."""
    key = (kind, n, d)
    if key not in _cases:
        X, y = O.synthetic_problem(n, d, 31)
        kp = params(kind, d)
        if n >= 128:
            st = engine.fit(t(X), t(y), kp)
            engine.inverse(st)
            torch.cuda.synchronize()
            _cases[key] = (kp, st.X, st.alpha[:, 0].contiguous(), st.W)
        else:
            g = torch.Generator(device="cpu").manual_seed(n * 100 + d)
            npad = int(engine.lib.gpx_padded_n(n))
            W = torch.triu(torch.randn(npad, npad, dtype=torch.float64, generator=g)).to(DEV)
            alpha = torch.randn(npad, dtype=torch.float64, generator=g).to(DEV)
            _cases[key] = (kp, t(X), alpha, W)
    return _cases[key]


def composition(engine, kp, X, alpha, Xs, W):
    """(ss of row tile 0, mean partials of row blocks 0 and 1) through the two launches' debug entries."""
    lib, n, d, m = engine.lib, X.shape[0], X.shape[1], Xs.shape[0]
    npad = int(lib.gpx_padded_n(n))
    ld = (m + 255) // 256 * 256
    K = torch.full((npad, ld), float("nan"), dtype=torch.float64, device=DEV)
    mu = torch.full((npad // 64, ld), float("nan"), dtype=torch.float64, device=DEV)
    pc = kp.to_c(d)
    _capi.check(lib.gpx_debug_kstar_mu_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha), ptr(Xs),
                                           m, Xs.stride(0), None, None, ptr(K), ld, ptr(mu), 0), engine.handle)
    ss = torch.full((npad // 128, ld), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_stage_product_workspace_size(ld, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    _capi.check(lib.gpx_debug_stage_product_f64(engine.handle, npad, ptr(W), W.stride(0), ptr(K), ld, ld, None, 0, 1, 0,
                                                ptr(ss), ld, ptr(ws), ws.numel()), engine.handle)
    torch.cuda.synchronize()
    return ss[0], mu[:2]


def head_product(engine, kp, X, alpha, Xs, W):
    lib, n, d, m = engine.lib, X.shape[0], X.shape[1], Xs.shape[0]
    ld = (m + 255) // 256 * 256
    ss = torch.full((ld,), float("nan"), dtype=torch.float64, device=DEV)
    mu = torch.full((2, ld), float("nan"), dtype=torch.float64, device=DEV)
    pc = kp.to_c(d)
    _capi.check(lib.gpx_debug_head_product_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha),
                                               ptr(Xs), m, Xs.stride(0), ptr(W), W.stride(0), ptr(ss), ptr(mu), ld),
                engine.handle)
    torch.cuda.synchronize()
    return ss, mu


# ---- (1) the kernel against the composition --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1000, 129])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [3, 8, 16])
@pytest.mark.parametrize("n", [40, 100, 300])
def test_bits_of_the_two_launches(engine, n, d, kind, m):
    kp, X, alpha, W = case(engine, kind, n, d)
    Xs = t(candidates(X.cpu().numpy(), m, np.random.default_rng(7 * n + d + m)))
    ss_ref, mu_ref = composition(engine, kp, X, alpha, Xs, W)
    ss, mu = head_product(engine, kp, X, alpha, Xs, W)
    nan_ref, nan_got = torch.isnan(ss_ref), torch.isnan(ss)
    print(f"n={n} d={d} {kind} m={m}: NaN columns {int(nan_ref.sum())}, "
          f"ss bit mismatches {int((bits(ss) != bits(ss_ref)).sum())}, "
          f"mu bit mismatches {int((bits(mu) != bits(mu_ref)).sum())}")
    assert torch.equal(nan_ref, nan_got)
    assert torch.equal(torch.isnan(mu_ref), torch.isnan(mu))
    assert int(nan_ref[:m].sum()) >= 1  # the NaN row reaches the sums
    assert not torch.isnan(ss_ref[m:]).any() and not torch.isnan(mu_ref).all()
    assert torch.equal(bits(ss), bits(ss_ref))
    assert torch.equal(bits(mu), bits(mu_ref))


def test_arguments_checked_on_a_live_handle(engine):
    kp, X, alpha, W = case(engine, "rbf", 300, 8)
    Xs = t(np.random.default_rng(1).random((129, 8)))
    lib, pc, bad = engine.lib, kp.to_c(8), _capi.GPX_INVALID_ARG
    out = torch.empty((3, 256), dtype=torch.float64, device=DEV)
    call = lambda W_, ldw, ldmu: lib.gpx_debug_head_product_f64(  # noqa: E731
        engine.handle, ctypes.byref(pc), 300, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), 129, 8, ptr(W_), ldw,
        ptr(out[0]), ptr(out[1:]), ldmu)
    assert call(W, W.stride(0), 128) == bad  # pitch below m rounded up to 256
    assert call(W, 256, 256) == bad          # W's pitch below padded n
    assert call(None, 384, 256) == bad
    assert call(W, W.stride(0), 256) == _capi.GPX_OK
    torch.cuda.synchronize()


# ---- (2) end to end --------------------------------------------------------------------------------------------------
N, D, K = 640, 8, 16
CALLS = [("rbf", "logei"), ("rbf", "ucb"), ("matern52", "logei")]


def fitted(engine, kind):
    if kind not in _fits:
        X, y = O.synthetic_problem(N, D, 21)
        kp = KernelParams(kind, botorch_default_lengthscale(D), noise=1e-4)
        _fits[kind] = (engine.fit(t(X), t(y), kp), float(y.max()))
    return _fits[kind]


def with_options(engine, head, fn):
    before = engine.get_option("sweep_prune"), engine.get_option("sweep_head")
    engine.set_option("sweep_prune", 2)
    engine.set_option("sweep_head", head)
    try:
        out = fn()
        stats = tuple(int(v) for v in engine.sweep_stats())
    finally:
        engine.set_option("sweep_prune", before[0])
        engine.set_option("sweep_head", before[1])
    return [bits(o).cpu() for o in out], stats


@pytest.mark.parametrize("m", [40_000, 5_000])
@pytest.mark.parametrize("kind,acq", CALLS)
def test_acquire_and_topk_under_both_heads(engine, kind, acq, m):
    st, best_f = fitted(engine, kind)
    Xs = t(O.sobol_candidates(m, D, 22))
    for name, fn in (("acquire", lambda: engine.acquire(st, Xs, acq, best_f=best_f)),
                     ("acquire_topk", lambda: engine.acquire_topk(st, Xs, K, acq, best_f=best_f))):
        fused, stats1 = with_options(engine, 1, fn)
        apart, stats0 = with_options(engine, 0, fn)
        print(f"{kind} {acq} m={m} {name}: sweep_stats fused {stats1} apart {stats0}")
        assert stats1[2] < stats1[3]  # the pruned path ran
        for a, b in zip(fused, apart):
            assert torch.equal(a, b), name
        assert stats1 == stats0, name


def test_option_defaults_to_the_fused_head(engine):
    assert engine.get_option("sweep_head") == 1
    with pytest.raises(Exception):
        engine.set_option("sweep_head", 2)
