"""gpx_svgp_acquire_f64 in exactly the bytes gpx_svgp_acquire_workspace_size reports, poisoned, at an 8-byte-aligned
address: tests/test_gpu_abi_workspace.py's check for the new call, through GPEngine.svgp_acquire with ``engine.workspace``
replaced (tests/abi_util.py GuardedWorkspace).  The results have the bits of the engine's call with its own workspace,
the bytes in front of the workspace and the 4 KiB behind it are still 0xFF, the engine asks for exactly what the size
query reports, and one byte less is rejected.  With and without scores_out (without: the workspace's own score array),
M = 200 (two row tiles) and M = 500 (where the sweep's layout carries its pruned part)."""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from tests import abi_util as A
from tests import svgp_moments_ref as SR
from tests.abi_util import GuardedWorkspace, same_bits, t
from tests.test_svgp import svgp_problem

pytestmark = pytest.mark.gpu
T, D, M, K = 2, 3, 700, 5


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("scores", [True, False], ids=["scores_out", "no_scores"])
@pytest.mark.parametrize("Mi", [200, 500])
def test_workspace_of_exactly_the_reported_size(engine, monkeypatch, Mi, scores, offset):
    Z, vmean, vchol, kps, _ = svgp_problem(T, Mi, D, seed=T + Mi, kind="rbf")
    prep = engine.svgp_prepare(kps, Z, vmean, vchol, jitter=SR.JITTER)
    Xn = t(np.random.default_rng(9).standard_normal((M, D)))
    size = A.ws_size(engine.lib.gpx_svgp_acquire_workspace_size, Mi, M, K)

    def run():
        return engine.svgp_acquire(prep, Xn, K, "ucb", beta=2.0, weights=[0.5, 1.0], y_mean=[0.1, 0.0],
                                   y_scale=[2.0, 1.0], return_scores=scores)

    want = run()
    torch.cuda.synchronize()
    short = GuardedWorkspace(offset, short_at=0)
    monkeypatch.setattr(engine, "workspace", short)
    with pytest.raises(_capi.GPXError, match="workspace too small") as e:
        run()
    assert e.value.status == _capi.GPX_INVALID_ARG
    assert short.guards_intact()
    guarded = GuardedWorkspace(offset)
    monkeypatch.setattr(engine, "workspace", guarded)
    got = run()
    assert guarded.guards_intact(), "a kernel wrote outside the reported workspace"
    assert guarded.asked == [size]
    assert len(got) == len(want) == (3 if scores else 2)
    for a, b in zip(got, want):
        assert same_bits(a, b), "differs from the run in the engine's workspace"
