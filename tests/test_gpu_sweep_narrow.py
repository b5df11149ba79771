"""The narrow (128 x 32) tile of the pruned sweep's staged product against the wide (128 x 128) one.

Yardstick: bit identity.  (1) gpx_debug_stage_product_f64 runs one stage in a named shape: the partials ss of the two
shapes are compared as int64 patterns, at padded n = 384 and 640 (three and five row tiles: the smallest sizes with the
stage widths 1, 1, 1 and 1, 1, 2, 1), over 32 / 33 / 128 / 200 / 300 columns (a whole narrow tile, one column into the
second, a whole wide tile, partial wide and narrow tiles, more than two wide tiles).  A float64 product bounds both.
(2) The argmax with sweep_prune = 2 against 0, on calls whose tail stages take the narrow shape, the wide one, and the
chunked form, with the sweep_stats the parent build reports for the same calls.  (3) The same call twice.
"""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NCOLS = [32, 33, 128, 200, 300]
NPADS = [384, 640]
WIDE, NARROW = 0, 1
_inputs = {}
_fits = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def ptr(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


def stages(nI):
    """The repository's stage boundaries 0 < 1 < 2 < 4 < 8 < 16 < nI as (I0, nrows)."""
    R = [0] + [r for r in (1, 2, 4, 8, 16) if r < nI] + [nI]
    return [(R[s], R[s + 1] - R[s]) for s in range(len(R) - 1)]


def inputs(npad):
    """(W upper triangular, K*) for one padded n, shared by the module and never modified."""
    if npad not in _inputs:
        g = torch.Generator(device="cpu").manual_seed(npad)
        W = torch.triu(torch.randn(npad, npad, dtype=torch.float64, generator=g)).to(DEV)
        K = torch.randn(npad, 384, dtype=torch.float64, generator=g).to(DEV)
        _inputs[npad] = (W, K, (W.T @ K) ** 2)
    return _inputs[npad]


def stage_product(engine, W, K, ncols, I0, nrows, shape, lst=None, ldss=None, expect=_capi.GPX_OK):
    """ss (nI rows, prefilled with NaN) after one call of gpx_debug_stage_product_f64."""
    lib, npad = engine.lib, W.shape[0]
    ldss = ldss or (ncols + 127) // 128 * 128
    ss = torch.full((npad // 128, ldss), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_stage_product_workspace_size(ncols, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    st = lib.gpx_debug_stage_product_f64(engine.handle, npad, ptr(W), W.stride(0), ptr(K), K.stride(0), ncols,
                                         ptr(lst), I0, nrows, shape, ptr(ss), ldss, ptr(ws), ws.numel())
    assert st == expect
    torch.cuda.synchronize()
    return ss


def bits(a):
    return a.contiguous().view(torch.int64)


# ---- (1) the two shapes through the debug entry ----------------------------------------------------------------------
@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("npad", NPADS)
def test_narrow_has_the_bits_of_wide(engine, npad, ncols):
    W, K, V2 = inputs(npad)
    nI, cpad = npad // 128, (ncols + 127) // 128 * 128
    ref = V2[:, :cpad].reshape(nI, 128, cpad).sum(1)
    for I0, nrows in stages(nI) + [(0, nI)]:
        wide = stage_product(engine, W, K, ncols, I0, nrows, WIDE)
        narrow = stage_product(engine, W, K, ncols, I0, nrows, NARROW)
        assert torch.equal(bits(wide), bits(narrow)), (I0, nrows)
        rows = torch.zeros(nI, dtype=torch.bool, device=DEV)
        rows[I0:I0 + nrows] = True
        assert torch.isnan(wide[~rows]).all()  # the other stages' rows stay untouched
        # 128 to 640 products per entry, summed in another order: 1e-12 relative is hundreds of roundings wide
        err = ((wide[rows] - ref[rows]).abs() / ref[rows]).max().item()
        assert err < 1e-12, (I0, nrows, err)


@pytest.mark.parametrize("npad", NPADS)
def test_column_list_with_padding(engine, npad):
    W, K, _ = inputs(npad)
    nI, ncols, ldss = npad // 128, 200, 512
    rng = np.random.default_rng(npad)
    cols = rng.permutation(ldss)[:ncols].astype(np.int32)
    pad = rng.permutation(ncols)[:9]
    cols[pad] = -1
    lst = torch.tensor(cols, device=DEV)
    plain = stage_product(engine, W, K, ncols, 0, nI, WIDE)
    live = np.flatnonzero(cols >= 0)
    for shape in (WIDE, NARROW):
        got = stage_product(engine, W, K, ncols, 0, nI, shape, lst, ldss)
        assert torch.equal(bits(got[:, cols[live]]), bits(plain[:, live]))
        untouched = np.setdiff1d(np.arange(ldss), cols[live])
        assert torch.isnan(got[:, untouched]).all()


@pytest.mark.parametrize("npad", NPADS)
def test_nan_column_stays_in_its_column(engine, npad):
    W, K, _ = inputs(npad)
    nI, ncols, bad = npad // 128, 200, 37
    Kn = K.clone()
    Kn[:, bad] = float("nan")
    clean = stage_product(engine, W, K, ncols, 0, nI, WIDE)
    others = [c for c in range(256) if c != bad]
    for shape in (WIDE, NARROW):
        got = stage_product(engine, W, Kn, ncols, 0, nI, shape)
        assert torch.isnan(got[:, bad]).all()
        assert torch.equal(bits(got[:, others]), bits(clean[:, others]))


def test_arguments_checked_on_a_live_handle(engine):
    W, K, _ = inputs(384)
    bad = _capi.GPX_INVALID_ARG
    stage_product(engine, W, K, 32, 0, 0, WIDE, expect=bad)      # nrows = 0
    stage_product(engine, W, K, 32, 2, 2, WIDE, expect=bad)      # I0 + nrows > nI
    stage_product(engine, W, K, 32, -1, 1, WIDE, expect=bad)
    stage_product(engine, W, K, 32, 0, 1, 2, expect=bad)         # unknown shape
    stage_product(engine, W, K, 300, 0, 1, NARROW, ldss=256, expect=bad)  # ss pitch below the padded column count
    lib = engine.lib
    assert lib.gpx_debug_stage_product_f64(engine.handle, 384, None, 384, ptr(K), 384, 32, None, 0, 1, 0, ptr(K), 128,
                                           ptr(K), 1 << 20) == bad  # W is NULL


# ---- (2) the argmax across the rule ----------------------------------------------------------------------------------
M = 5000
COPIES = 40_000  # of the best candidate: 313 wide tiles in every tail stage, more than one tile row of the device
# sweep_stats of the sweep_prune = 2 call of each case on the parent build (commit 5237ef2, the wide tile throughout),
# read on an MI355X through GPX_LIB with this file's case() inputs.  Product tiles are counted in 128 x 128 units in
# either shape, so all four numbers must match.
PARENT_STATS = {
    "sparse": (5000, 1032, 87, 200),
    "dense": (45000, 42195, 1672, 1760),
    "chunked": (5000, 1031, 58, 120),
}


def fitted(engine, n, d):
    if (n, d) not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams("rbf", botorch_default_lengthscale(d), noise=1e-4)
        _fits[(n, d)] = (engine.fit(t(X), t(y), kp), float(y.max()))
    return _fits[(n, d)]


def acquire(engine, prune, st, Xs, best_f):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        bv, bi = engine.acquire(st, Xs, "logei", best_f=best_f)
        stats = tuple(int(v) for v in engine.sweep_stats())
    finally:
        engine.set_option("sweep_prune", before)
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def case(engine, name):
    """(state, candidates, best_f) of a named call.
    sparse: the n = 640, 5000-candidate Sobol problem of the prune tests (a few survivors per tail stage: narrow tiles).
    dense: the same followed by COPIES copies of its best candidate, none of which can be dropped (wide tiles).
    chunked: d = 20 at n = 384 (no lazy form above d = 16: launch_sweep_chunk_pruned)."""
    if name == "chunked":
        st, best_f = fitted(engine, 384, 20)
        return st, t(O.sobol_candidates(M, 20, 22)), best_f
    st, best_f = fitted(engine, 640, 4)
    Xs = O.sobol_candidates(M, 4, 22)
    if name == "dense":
        i0 = acquire(engine, 0, st, t(Xs), best_f)[1]
        Xs = np.concatenate([Xs, np.repeat(Xs[i0:i0 + 1], COPIES, axis=0)])
    return st, t(Xs), best_f


@pytest.mark.parametrize("name", list(PARENT_STATS))
def test_argmax_bits_and_parent_stats(engine, name):
    if name == "dense":
        assert torch.cuda.get_device_properties(0).multi_processor_count * 128 < COPIES
    st, Xs, best_f = case(engine, name)
    full = acquire(engine, 0, st, Xs, best_f)
    pruned = acquire(engine, 2, st, Xs, best_f)
    again = acquire(engine, 2, st, Xs, best_f)
    print(f"{name}: sweep_stats pruned {pruned[2]} full {full[2]}")
    assert pruned[:2] == full[:2], (pruned, full)
    assert pruned[2][2] < pruned[2][3]  # the staged path ran
    assert again == pruned              # (3) the same call twice: bits and stats
    assert pruned[2] == PARENT_STATS[name]
