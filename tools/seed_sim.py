"""CPU simulation of the seeded order of the lazy pruned sweep, NumPy fp64, exact means in place of the
mean bound, on bench.py's problem (n = 4096, d = 8, RBF, logEI, 2^20 Sobol candidates) or another seed's.

Per problem seed: the head's score bound U of every candidate (exact mean, the variance left after the product's first
128 rows), the incumbent the leading 1,024 candidates give and how many columns of the old first span (one chunk) and
of the whole call its bound pass keeps, then the same for the seed made of the arg max of U in each of 1,024 slices.
One JSON line per seed.  No GPU.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.linalg as sla
from bayesianoptimizer_amd import synthetic
from oracle import gp_oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", default="0,1000")
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--m", type=int, default=1 << 20)
a = ap.parse_args()
D, SEED, EPS = 8, 1024, 1e-9


def keeps(U, tau):  # the bound passes' test (bound_keeps in gpx_sweep.hip)
    return ~(U + EPS * (np.abs(U) + abs(tau) + 1.0) < tau)


for seed in (int(s) for s in a.seeds.split(",")):
    X, y = synthetic.problem(a.n, D, seed)
    Xs = synthetic.sobol(a.m, D, seed + 1)
    kp = O.KernelParams(O.RBF, np.full(D, O.botorch_default_lengthscale(D)), noise=1e-4)
    st = O.fit(X, y, kp)
    best_f = float(y.max())
    L0 = st.L[:128, :128]
    U = np.empty(a.m)
    for c in range(0, a.m, 1 << 15):
        P = Xs[c:c + (1 << 15)]
        K = O.kernel_matrix(X, P, kp)
        v0 = sla.solve_triangular(L0, K[:128], lower=True, check_finite=False)
        mu = kp.const_mean + st.alpha @ K
        U[c:c + (1 << 15)] = O.acquisition(mu, np.maximum(O.kernel_diag(P, kp) - (v0 * v0).sum(0), 1e-10), O.ACQ_LOGEI,
                                           best_f)

    def exact(idx):
        return O.acquisition(*O.posterior(st, Xs[idx]), O.ACQ_LOGEI, best_f)

    C = ((1 << 30) // 8 // ((a.n + 127) // 128 * 128)) // 256 * 256
    lead = exact(np.arange(SEED))
    tau0 = float(lead.max())
    pick = np.array([s * a.m // SEED + int(np.argmax(U[s * a.m // SEED:(s + 1) * a.m // SEED])) for s in range(SEED)])
    sc = exact(pick)
    tau1 = float(sc.max())
    k1 = keeps(U, tau1)
    k1[pick] = False
    print(json.dumps({"seed": seed, "tau_leading_block": tau0,
                      "first_span_head_survivors_leading_block": int(keeps(U[1024:C], tau0).sum()),
                      "tau_slice_seed": tau1, "its_index": int(pick[int(np.argmax(sc))]),
                      "argmax_U": int(np.argmax(U)), "head_survivors_slice_seed_all": int(keeps(U, tau1).sum()),
                      "head_survivors_outside_the_seed": int(k1.sum())}), flush=True)
