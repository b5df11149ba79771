"""The lazy pruned sweep's tail with the survivor count read back (sweep_tail_sync = 1): a span that can need
more than one round of C survivors copies its count to the host, enqueues round 0, waits, and enqueues only the rounds
the count needs; sweep_tail_sync = 0 enqueues the worst case, as before.

Yardstick: bit identity of (best_val, best_idx), of every top-k pair and of sweep_stats between the two settings, and of
value and index against sweep_prune = 0; gpx_debug_get_tail_rounds (rounds enqueued, worst case, sum of the counts read
back) as named at each test.  Shapes: the smallest with more than one round, padded n = 384 (n = 300, d = 4, RBF), whose
chunk is C = 2^27 / 384 = 349 440 columns: m = 400 000 is one span of 2 rounds, m = 1 100 000 a span of 2^20 columns
(4 rounds) and one of 51 424 (1 round, no read-back); m = 100 000 is a single round.  One fit and one Sobol set for the
module, never modified.

Survivor counts of the first span read back on an MI355X with this file's inputs (the same under sweep_order 1 and 0),
m = 400 000 / m = 1 100 000, against C = 349 440:
    acquire: logei 0 / 0, ei 0 / 0, ucb 1 / 15
    acquire_topk, k = 1, 16, 1024: logei 0, 0, 11 918 / 0, 0, 2 656; ei 0, 0, 11 927 / 0, 0, 2 656;
                                   ucb 1, 4, 6 419 / 15, 28, 9 576
so every one of these calls enqueues one round per span (2 of 5 at m = 1 100 000, 1 of 2 at m = 400 000).  m = 400 000
identical candidates: 398 976 (every column but the seed's 1024), both rounds.
"""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, D = 300, 4
C = 349_440          # sweep_chunk_size(384, m) of every m >= C
SUPER = 1 << 20
SEED = 1024          # PRUNE_SEED: the seeded span's seed columns are scored apart and are no survivors
M_ONE, M_TWO, M_SPANS = 100_000, 400_000, 1_100_000
WORST = {M_ONE: 1, M_TWO: 2, M_SPANS: 4 + 1}
SPANS = {M_ONE: 1, M_TWO: 1, M_SPANS: 2}
_cache = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def bits(a):
    return a.contiguous().view(torch.int64)


def fitted(engine):
    """(state, best_f) of the module's one fit."""
    if "fit" not in _cache:
        X, y = O.synthetic_problem(N, D, 21)
        kp = KernelParams("rbf", botorch_default_lengthscale(D), noise=1e-4)
        _cache["fit"] = (engine.fit(t(X), t(y), kp), float(y.max()))
    return _cache["fit"]


def host_candidates():
    if "host" not in _cache:
        _cache["host"] = O.sobol_candidates(M_SPANS, D, 22)
    return _cache["host"]


def candidates(m):
    """The leading m of the module's Sobol set, on the device."""
    if m not in _cache:
        _cache[m] = t(host_candidates()[:m])
    return _cache[m]


def identical(m):
    return t(np.repeat(host_candidates()[17:18], m, axis=0))


def run(engine, prune, order, sync, fn):
    """fn() under the three options: (its tensors' bits and values, sweep_stats, tail rounds)."""
    names = ("sweep_prune", "sweep_order", "sweep_tail_sync")
    before = [engine.get_option(k) for k in names]
    for k, v in zip(names, (prune, order, sync)):
        engine.set_option(k, v)
    try:
        out = fn()
        rounds = engine.tail_rounds()  # (host-side: read before sweep_stats synchronises)
        stats = tuple(int(v) for v in engine.sweep_stats())
    finally:
        for k, v in zip(names, before):
            engine.set_option(k, v)
    val, idx = out
    return (tuple(bits(val).tolist()), tuple(idx.tolist())), stats, rounds


def both(engine, order, fn, m):
    """fn() with the read-back on and off: equal bits, equal sweep_stats; the off run enqueues the worst case and reads
    nothing back, the on run what its count needs.  Returns (result, rounds of the on run)."""
    on, on_stats, on_rounds = run(engine, 1, order, 1, fn)
    off, off_stats, off_rounds = run(engine, 1, order, 0, fn)
    print(f"m = {m} order {order}: tail rounds on {on_rounds} off {off_rounds}; sweep_stats on {on_stats} off {off_stats}")
    assert on == off
    assert on_stats == off_stats
    assert off_rounds == (WORST[m], WORST[m], -1)
    assert on_rounds[1] == WORST[m]
    if m == M_ONE:
        assert on_rounds == (1, 1, -1)
    else:
        # every multi-round span here is the call's first: its rounds from its own count, one more for a second span
        count = on_rounds[2]
        first = min(m, SUPER)
        assert 0 <= count <= first
        assert on_rounds[0] == min(-(-first // C), max(1, -(-count // C))) + (SPANS[m] - 1)
    return on, on_rounds


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [M_TWO, M_SPANS])
@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("acq", ["logei", "ei", "ucb"])
def test_equal_bits_with_and_without_the_read_back(engine, acq, order, m):
    st, best_f = fitted(engine)
    Xs = candidates(m)
    kw = dict(best_f=best_f, beta=4.0)
    got, _ = both(engine, order, lambda: engine.acquire(st, Xs, acq, **kw), m)
    full, full_stats, full_rounds = run(engine, 0, order, 1, lambda: engine.acquire(st, Xs, acq, **kw))
    assert full_stats[1] == m and full_rounds == (0, 0, -1)  # (the full sweep: no tail)
    assert got == full
    _, _, sc = engine.acquire(st, Xs, acq, return_scores=True, **kw)
    for k in (1, 16, 1024):
        v_ref, i_ref = engine.topk(sc, k)
        got, _ = both(engine, order, lambda: engine.acquire_topk(st, Xs, k, acq, **kw), m)
        assert got == (tuple(bits(v_ref).tolist()), tuple(i_ref.tolist())), k


# ---- 2. the rounds that were enqueued ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [M_TWO, M_SPANS])
@pytest.mark.parametrize("order", [1, 0])
def test_one_round_per_span(engine, order, m):
    """logEI on the Sobol set leaves far fewer survivors than a chunk holds, so the read-back enqueues one round per
    span, and without it the worst case runs.  On an MI355X the count read back is 0 at both sizes and under both
    orders: the seed's incumbent prunes every other column of the first span."""
    st, best_f = fitted(engine)
    Xs = candidates(m)
    _, rounds = both(engine, order, lambda: engine.acquire(st, Xs, "logei", best_f=best_f), m)
    assert 0 <= rounds[2] <= C
    assert rounds == (SPANS[m], WORST[m], rounds[2])


def test_a_single_round_reads_nothing_back(engine):
    st, best_f = fitted(engine)
    Xs = candidates(M_ONE)
    for order in (1, 0):
        _, rounds = both(engine, order, lambda: engine.acquire(st, Xs, "logei", best_f=best_f), M_ONE)
        assert rounds == (1, 1, -1)
        _, rounds = both(engine, order, lambda: engine.acquire_topk(st, Xs, 16, "logei", best_f=best_f), M_ONE)
        assert rounds == (1, 1, -1)


# ---- 3. later rounds that are live -------------------------------------------------------------------------------------
def test_identical_candidates_keep_every_round(engine):
    """Nothing prunable: every column but the seed's survives, the second round is live and must be enqueued."""
    st, best_f = fitted(engine)
    m = M_TWO
    Xs = identical(m)
    fn = lambda: engine.acquire(st, Xs, "logei", best_f=best_f, index_offset=11)  # noqa: E731
    got, rounds = both(engine, 1, fn, m)
    full, full_stats, _ = run(engine, 0, 1, 1, fn)
    assert got == full and got[1] == (11,)
    assert rounds[0] == rounds[1] == 2 and rounds[2] > C
    _, stats, _ = run(engine, 1, 1, 1, fn)
    assert stats[1] == m and stats[2] == stats[3] == full_stats[3]


# ---- 4. the boundary ---------------------------------------------------------------------------------------------------
def test_count_of_exactly_a_chunk_and_one_more(engine):
    """Identical candidates, m around C: a count of exactly C fills round 0 and needs no second round, C + 1 needs it.
    Every column but the seed's SEED survives, so m = C + SEED gives C; the test reads the count the first call reports
    and moves m by the difference, so that the two calls it asserts on have exactly C and C + 1."""
    st, best_f = fitted(engine)
    results = {}

    def call(m):
        Xs = identical(m)
        fn = lambda: engine.acquire(st, Xs, "logei", best_f=best_f)  # noqa: E731
        on, on_stats, on_rounds = run(engine, 1, 1, 1, fn)
        off, off_stats, off_rounds = run(engine, 1, 1, 0, fn)
        print(f"m = {m}: tail rounds on {on_rounds} off {off_rounds}")
        assert on == off and on_stats == off_stats and off_rounds == (2, 2, -1)
        results[m] = on
        return on_rounds

    m0 = C + SEED
    shift = call(m0)[2] - C  # 0 when exactly the seed's columns are no survivors
    assert abs(shift) < SEED + 256, shift
    at, above = call(m0 - shift), call(m0 - shift + 1)
    assert at == (1, 2, C)
    assert above == (2, 2, C + 1)
    assert len({r for r in results.values()}) == 1  # the same candidate everywhere: index 0, one value


# ---- 5. the switch -----------------------------------------------------------------------------------------------------
def test_switch_defaults_to_the_read_back_and_rejects_other_values(engine):
    assert engine.get_option("sweep_tail_sync") == 1
    for bad in (2, -1):
        assert engine.lib.gpx_debug_set_sweep_tail_sync(engine.handle, bad) == _capi.GPX_INVALID_ARG
        with pytest.raises(_capi.GPXError) as err:
            engine.set_option("sweep_tail_sync", bad)
        assert err.value.status == _capi.GPX_INVALID_ARG
    assert engine.get_option("sweep_tail_sync") == 1
    engine.set_option("sweep_tail_sync", 0)
    assert engine.get_option("sweep_tail_sync") == 0
    engine.set_option("sweep_tail_sync", 1)
