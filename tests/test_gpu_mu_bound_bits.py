"""The head mean bound keeps its bits (gpx_mubound.hip): gpx_debug_mu_bound_f64's mu_approx, mu_slack and its two
counters against tests/golden/mu_bound_bits.json, recorded from the commit before the bound moved into its own unit and
its two factorised loops became one body.

Shapes (n, d): (300, 3) and (300, 16) (the fp64 factorised form and mu_bound_kernel, DMAX 4 and 16), (300, 5) and
(300, 8) (all three forms at DMAX 8), (640, 8) (ten row blocks); the 3000 mixed candidates of tests/mu_bound_util.py (a
partial last workgroup, one NaN and one infinite candidate).  alpha is made on the host from a seeded generator, so the
fixture depends on no other kernel: Gaussian, magnitudes over a range of 2^200, and a one-hot.  Per case the fixture
holds the sha256 of the inputs' bytes (checked first: a mismatch there is the host's, not the kernels'), of mu_approx's
and of mu_slack's, and the counters.  To record it again:

    python tests/test_gpu_mu_bound_bits.py OUT.json
"""
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.mu_bound_util import mixed_candidates, mu_bound, t

pytestmark = pytest.mark.gpu
SHAPES = [(300, 3), (300, 5), (300, 8), (640, 8), (300, 16)]
ALPHAS = ["gaussian", "2^200 range", "one-hot"]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mu_bound_bits.json")
_inputs = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs(n, d):
    """X, the mixed candidates and the three alphas (zero on the padded rows) of a shape, once per module."""
    if (n, d) not in _inputs:
        X, _ = O.synthetic_problem(n, d, 21)
        ls = botorch_default_lengthscale(d)
        rng = np.random.default_rng(1000 * n + d)
        Xs = mixed_candidates(X, ls, rng)[0]
        npad = (n + 127) // 128 * 128
        alphas = {name: np.zeros(npad) for name in ALPHAS}
        alphas["gaussian"][:n] = 30.0 * rng.standard_normal(n)
        mag = np.ldexp(1.0 + rng.random(n), -rng.integers(0, 200, n).astype(np.int32))
        mag[0], mag[1] = 1.0, 2.0 ** -200
        alphas["2^200 range"][:n] = mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        alphas["one-hot"][77] = -2.5
        _inputs[(n, d)] = (X, Xs, KernelParams("rbf", ls, outputscale=1.3), alphas)
    return _inputs[(n, d)]


def digest(engine, n, d, name):
    X, Xs, kp, alphas = inputs(n, d)
    alpha = alphas[name]
    ma, sl, fallback, fp64form = mu_bound(engine, kp, t(X), t(alpha), t(Xs))
    return {"inputs_sha256": sha(np.concatenate([X.ravel(), Xs.ravel(), alpha])),
            "mu_approx_sha256": sha(ma.cpu().numpy()), "mu_slack_sha256": sha(sl.cpu().numpy()),
            "fallback": fallback, "fp64form": fp64form}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ALPHAS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_mu_bound_bits(engine, golden, n, d, name):
    want = golden[f"n={n} d={d} alpha {name}"]
    got = digest(engine, n, d, name)
    assert got["inputs_sha256"] == want["inputs_sha256"], "the host-made inputs differ from the recorded ones"
    assert got == want


if __name__ == "__main__":
    from bayesianoptimizer_amd import GPEngine

    eng = GPEngine(0)
    out = {f"n={n} d={d} alpha {name}": digest(eng, n, d, name) for n, d in SHAPES for name in ALPHAS}
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} cases -> {sys.argv[1]}")
