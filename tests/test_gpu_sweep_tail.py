"""The tail of the pruned sweep: bounded grids whose workgroups divide the live work among themselves (the
gather strides over its units, the compaction splits each slot block's rows).

Yardstick: (value bits, index) with sweep_prune = 2 against 0 and the sweep_stats identities of test_gpu_sweep_lazy.py.
Shapes: padded n = 384 and 640, the smallest with 3 and 5 row tiles, d = 4 or 8.  A tail launch has a bounded grid (the
gather twice its resident workgroups, for the d = 8 instance 8 per CU: 2,048 on 256 CUs; the compaction 8 per CU).  At
n = 640 the gather has 10 row blocks per 256 columns, so 58,976 live columns give 2,310 units: a second trip for 262
workgroups, and 20,000 columns give 790 units: fewer than workgroups.
The compaction splits each 256-slot block's rows over gridDim / blocks workgroups; the cases here cover 1 to 410
blocks (half a chunk at n = 640).

The candidate sets are a scrambled Sobol set with a block of copies of its best candidate put in front of the original:
the copies share its score bits, survive every stage, and the lowest index among them wins.  The set's best and worst
candidates come from the CPU oracle's scores (one evaluation per set for the module), the best checked against the full
sweep on the device.  The lazy form's head phase, which bounds the mean as well, leaves about 45 of 39,000 Sobol
candidates to the tail, so a compaction of many columns cannot be built there: those cases run the chunked form of the
same staged driver (cov_fp32: launch_sweep_chunk_pruned), whose first stage runs in place on the chunk's K* and whose
first compaction moves the survivors with the same kernel.

The descriptors of the last chunk's or round's stages are still in the workspace after a call; the tests read them
there to assert the path a call took (slot s: the column set of stage s of a chunk, or with the lazy form slot 0 the
head's set, slot 1 the gather's, then one per compaction).
"""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED_BLOCK = 1024
CHUNK_640 = 209_664
_fits = {}
_sets = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, d, cov_fp32=False):
    """One fit per configuration for the whole module, on the device and in the oracle; never modified."""
    if (n, d, cov_fp32) not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        ls = botorch_default_lengthscale(d)
        st = engine.fit(t(X), t(y), KernelParams("rbf", ls, noise=1e-4, cov_fp32=cov_fp32))
        ost = O.fit(X, y, O.KernelParams(O.RBF, np.full(d, ls), noise=1e-4))
        _fits[(n, d, cov_fp32)] = (st, ost, float(y.max()))
    return _fits[(n, d, cov_fp32)]


def sobol_set(engine, n, d, m, cov_fp32=False):
    """(candidates, index of the best, index of the worst) by the oracle's scores, the best checked on the device."""
    if (n, d, m, cov_fp32) not in _sets:
        st, ost, best_f = fitted(engine, n, d, cov_fp32)
        base = O.sobol_candidates(m, d, 22)
        _, i_best, scores = O.acquire_argmax(ost, base, O.ACQ_LOGEI, best_f=best_f)
        assert acquire(engine, 0, st, t(base), best_f)[1] == i_best
        assert i_best >= SEED_BLOCK, "the set's best lies in the seed block: choose another seed"
        _sets[(n, d, m, cov_fp32)] = (base, int(i_best), int(np.argmin(scores)))
    return _sets[(n, d, m, cov_fp32)]


def acquire(engine, prune, st, Xs, best_f):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        bv, bi = engine.acquire(st, Xs, "logei", best_f=best_f)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def both(engine, st, Xs, best_f):
    full = acquire(engine, 0, st, Xs, best_f)
    pruned = acquire(engine, 2, st, Xs, best_f)
    print(f"sweep_stats pruned {pruned[2]} full {full[2]}")
    assert pruned[:2] == full[:2], (pruned, full)
    m = Xs.shape[0]
    assert full[2][0] == m and full[2][1] == m and full[2][2] == full[2][3] > 0
    assert pruned[2][0] == m and pruned[2][3] == full[2][3]
    return full, pruned


def with_copies(base, i_best, ncopy, start):
    """base with ncopy copies of its best candidate inserted at `start` (behind the seed block, before the original)."""
    assert SEED_BLOCK <= start <= i_best
    return np.concatenate([base[:start], np.repeat(base[i_best:i_best + 1], ncopy, axis=0), base[start:]])


def stage_descriptors(engine, npad, m):
    """(descriptors, survivor counts) of the last call's workspace: per slot (buf, col0, ncols, ntiles, list)."""
    ws = engine._ws["sweep"]
    cap = ((1 << 30) // 8 // npad) // 256 * 256
    C = min((m + 255) // 256 * 256, cap)
    nrec = (m + 255) // 256 + 1
    main = npad * C * 8 + (npad // 64) * C * 8 + (npad // 128) * C * 8 + 2 * nrec * 8
    at = (-ws.data_ptr()) % 256 + (main + 255) // 256 * 256
    torch.cuda.synchronize()
    desc = ws[at:at + 256].view(torch.int32).reshape(8, 8)[:, :5].tolist()
    count = ws[at + 256:at + 288].view(torch.int32).tolist()
    print("descriptors", desc[:4], "counts", count[:4])
    return desc, count


# ---- 1. more than one trip of the gather ---------------------------------------------------------------------------
def test_unprunable_round_with_more_gather_units_than_the_grid(engine):
    st, _, best_f = fitted(engine, 640, 8)
    m = 60_000
    Xs = t(np.repeat(O.sobol_candidates(64, 8, 22)[17:18], m, axis=0))
    full, pruned = both(engine, st, Xs, best_f)
    assert full[1] == 0
    assert pruned[2][1] == m and pruned[2][2] == pruned[2][3]
    d, _ = stage_descriptors(engine, 640, m)
    ntl = (m - SEED_BLOCK + 127) // 128
    assert d[1] == [0, 0, m - SEED_BLOCK, ntl, 2]
    assert d[2] == d[1] and d[3] == d[1]  # nothing dropped: every stage keeps the round's buffer


# ---- 2. large compactions ------------------------------------------------------------------------------------------
def test_lazy_block_of_copies(engine):
    """40,000 Sobol candidates and 20,000 copies of the best through the lazy form: 790 gather units; the copies and
    the few Sobol survivors of the head stay in the round's buffer through every stage."""
    st, _, best_f = fitted(engine, 640, 8)
    base, i_best, _ = sobol_set(engine, 640, 8, 40_000)
    start = min(i_best, 30_000)
    Xs = with_copies(base, i_best, 20_000, start)
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == start
    assert pruned[2][1] >= 20_000 and pruned[2][2] < pruned[2][3]
    d, _ = stage_descriptors(engine, 640, Xs.shape[0])
    for k in (1, 2, 3):
        assert d[k][0] == 0 and d[k][2] >= 20_000 and d[k][3] == (d[k][2] + 127) // 128


def test_chunked_compaction_of_a_third_of_a_chunk(engine):
    """The same set through the chunked form: its first stage runs in place on 58,976 columns, the copies and a few
    others survive it (less than half), and the first compaction moves at least 20,000 columns: 79 blocks of slots,
    each block's 640 rows split over 25 workgroups."""
    st, _, best_f = fitted(engine, 640, 8, True)
    base, i_best, _ = sobol_set(engine, 640, 8, 40_000, True)
    start = min(i_best, 30_000)
    Xs = with_copies(base, i_best, 20_000, start)
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == start
    assert pruned[2][1] >= 20_000 and pruned[2][2] < pruned[2][3]
    d, c = stage_descriptors(engine, 640, Xs.shape[0])
    assert d[0] == [0, SEED_BLOCK, 60_000 - SEED_BLOCK, (60_000 - SEED_BLOCK + 127) // 128, -1]
    assert 20_000 <= c[0] <= (60_000 - SEED_BLOCK) // 2
    assert d[1] == [1, 0, c[0], (c[0] + 127) // 128, 0]


def test_chunked_compaction_of_exactly_half_a_chunk(engine):
    """The largest set a compact buffer must hold: a later chunk of a call (no seed block: C staged columns) whose first
    half are copies of the best candidate and whose second half copies of the worst.  The survivors fill the compact
    buffer to its last column: 410 blocks of slots, each block's rows split over 4 workgroups."""
    st, _, best_f = fitted(engine, 640, 8, True)
    base, i_best, i_worst = sobol_set(engine, 640, 8, 40_000, True)
    C = CHUNK_640
    Xs = np.repeat(base[i_worst:i_worst + 1], 2 * C, axis=0)
    Xs[:SEED_BLOCK] = base[:SEED_BLOCK]
    Xs[500] = base[i_best]
    Xs[C:C + C // 2] = base[i_best]
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == 500
    assert pruned[2][1] == SEED_BLOCK + C // 2
    d, c = stage_descriptors(engine, 640, 2 * C)
    assert d[0] == [0, 0, C, C // 128, -1] and c[0] == C // 2
    assert d[1] == [1, 0, C // 2, C // 256, 0]
    assert d[2] == d[1] and d[3] == d[1]


# ---- 3. rounds of a few tiles through the whole call --------------------------------------------------------------------
@pytest.mark.parametrize("ncopy", [100, 200, 300, 500, 129, 50, 420])
def test_few_tiles(engine, ncopy):
    """50 Sobol candidates of this set survive the head, so the round has ncopy + 50 columns: 2, 2, 3, 5 and 2 tiles
    (179 columns: no multiple of 128) for the first five counts; 50 and 420 copies add the rounds of 1 and 4 tiles."""
    st, _, best_f = fitted(engine, 384, 4)
    base, i_best, _ = sobol_set(engine, 384, 4, 20_000)
    Xs = with_copies(base, i_best, ncopy, SEED_BLOCK + 77)
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == SEED_BLOCK + 77
    d, _ = stage_descriptors(engine, 384, Xs.shape[0])
    assert d[1][2] >= ncopy and d[1][:2] == [0, 0] and d[1][3:] == [(d[1][2] + 127) // 128, 2]
    assert d[2][2] >= ncopy and d[2][3] == (d[2][2] + 127) // 128


# ---- 4. a stage that keeps its buffer, then one that compacts ------------------------------------------------------
def test_kept_buffer_then_compaction(engine):
    """Copies survive every stage, so a set can be kept at one stage and compacted at a later one only through the other
    candidates dying in between: with h others in the round, s1 of them left after its first stage and s2 after its
    second, k copies are kept first and moved second when h - 2 s1 < k <= h - 2 s2.  The 40,000-candidate set at padded
    n = 640 has h = 45, s1 = 21, s2 = 15 (its own run, without copies, compacts at once), so 3 < k <= 15: k = 8."""
    st, _, best_f = fitted(engine, 640, 8)
    base, i_best, _ = sobol_set(engine, 640, 8, 40_000)
    Xs = with_copies(base, i_best, 8, SEED_BLOCK + 5)
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == SEED_BLOCK + 5
    d, c = stage_descriptors(engine, 640, Xs.shape[0])
    assert d[2] == d[1], "the first compaction did not keep the buffer"
    assert d[3] == [1, 0, c[2], 1, 0] and 2 * c[2] <= d[2][2]


# ---- 5. a round with zero survivors --------------------------------------------------------------------------------
def test_round_with_zero_survivors(engine):
    st, _, best_f = fitted(engine, 640, 8)
    base, i_best, i_worst = sobol_set(engine, 640, 8, 40_000)
    Xs = np.repeat(base[i_worst:i_worst + 1], 20_000, axis=0)
    Xs[:SEED_BLOCK] = base[:SEED_BLOCK]
    Xs[500] = base[i_best]
    full, pruned = both(engine, st, t(Xs), best_f)
    assert full[1] == 500
    assert pruned[2][1] == SEED_BLOCK
    d, _ = stage_descriptors(engine, 640, Xs.shape[0])
    assert d[1] == [0, 0, 0, 0, 2]


# ---- 6. the gather build against the full build --------------------------------------------------------------------
def debug_kstar(engine, kp, X, Xs, m, list_=None, count=None):
    lib, n, d = engine.lib, X.shape[0], X.shape[1]
    npad = int(lib.gpx_padded_n(n))
    ld = (m + 255) // 256 * 256
    out = torch.full((npad, ld), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_kstar_workspace_size(n, ld, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    pc = kp.to_c(d)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
    st = lib.gpx_debug_kstar_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(Xs), m, Xs.stride(0),
                                 ptr(list_), ptr(count), ptr(out), ld, ptr(ws), ws.numel())
    _capi.check(st, engine.handle)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cnt", [0, 1, 128, 129])
def test_gather_build_against_full_build(engine, cnt):
    n, d, m, cap = 600, 8, 3000, 1500  # padded n = 640 (40 padded rows)
    rng = np.random.default_rng(3)
    X, _ = O.synthetic_problem(n, d, 21)
    Xs = rng.random((m, d))
    kp = KernelParams("rbf", list(0.3 + rng.random(d)), outputscale=1.3)
    idx = rng.permutation(m)[:cap].astype(np.int32)
    Xd, Xsd = t(X), t(Xs)
    full = debug_kstar(engine, kp, Xd, Xsd, m)
    lst = torch.tensor(idx, dtype=torch.int32, device=DEV)
    got = debug_kstar(engine, kp, Xd, Xsd, cap, lst, torch.tensor([cnt], dtype=torch.int32, device=DEV))
    want = full.view(torch.int64)[:, torch.tensor(idx[:cnt].astype(np.int64), device=DEV)]
    assert torch.equal(got.view(torch.int64)[:, :cnt], want)
    assert torch.all(got[:, cnt:(cnt + 127) // 128 * 128] == 0)
    assert torch.isnan(got[:, (cnt + 255) // 256 * 256:]).all()  # nothing beyond the last live workgroup's columns
