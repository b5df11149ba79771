"""Time of one evaluation of qNoisyExpectedImprovement / qLogNoisyExpectedImprovement under optimize_acqf, split into
its three device parts, against the same chain in torch, on a fitted exact GP (default n = 1024, d = 8 Matern-5/2,
nb = 32 baseline points, S = 512 base samples):

  grad_B5_q4    acq(X) and d/dX at B = 5 (batch_limit) q-batches of q = 4: one L-BFGS-B evaluation
  score_1024_q4 value-only scoring of 1024 raw q-batches of q = 4 (gen_batch_initial_conditions)

Parts: ``moments`` (gpx_moments_grad_f64 and its chain rule, shared by both arms), ``cross`` (gpx_cross_cov_grad_f64 and
its chain rule, against the kernel evaluated with torch operations and differentiated by autograd) and ``mc``
(gpx_mc_nei_f64, against batched cholesky_ex with its host read, einsum, amax / relu or the log chains and autograd
backward, on precomputed moments); ``whole`` is the acquisition object's call.  The arms alternate in one process; every
figure is the median of --reps device-event timings (the events bracket the whole step, host gaps and the torch arm's
synchronisation included) after --warmup evaluations.  Prints one JSON line per shape and acquisition."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bayesianoptimizer_amd import KernelParams, acqf, synthetic
from bayesianoptimizer_amd.models import ExactGP
from bayesianoptimizer_amd.transforms import Standardize

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--baseline", type=int, default=32)
ap.add_argument("--samples", type=int, default=512)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mc_nei_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)

X, y = synthetic.problem(a.n, a.d, seed=0)
LS, NOISE = 0.5, 1e-3
gp = ExactGP(X, y.reshape(-1, 1), KernelParams("matern52", LS, noise=NOISE), outcome_transform=Standardize()).fit()
best_rows = np.argsort(-y)[: a.baseline]  # the baseline: the best observed points, unpruned so that nb is as asked
Xb = torch.tensor(X[np.sort(best_rows)], device=dev)
acqs = {log: (acqf.qLogNoisyExpectedImprovement if log else acqf.qNoisyExpectedImprovement)(
    gp, Xb, sampler=acqf.SobolQMCNormalSampler(torch.Size([a.samples]), 11), prune_baseline=False) for log in (0, 1)}
obj = acqs[0].objective
(st, _, _, vs), = obj.terms
Xtrain = st.X[: st.n]
rng = np.random.default_rng(1)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def matern52(A, B):
    r = torch.cdist(A / LS, B / LS)
    s5r = math.sqrt(5.0) * r
    return st.params.outputscale * (1.0 + s5r + (5.0 / 3.0) * r * r) * torch.exp(-s5r)


def cross_gpx(acq, Xs):
    Sb = acq._baseline[3][0]
    return vs * acqf._Cross.apply(Xs, gp.engine, st, Sb, acq.X_baseline)


def cross_torch(acq, Xs):
    Sb = acq._baseline[3][0]
    return vs * (matern52(Xs, acq.X_baseline) - matern52(Xs, Xtrain) @ Sb[: st.n, : acq.X_baseline.shape[0]])


def mc_gpx(acq, mu, cov, cross, setup):
    return acqf._McNei.apply(mu, cov, cross, gp.engine, setup, acq._opts())


def mc_torch(acq, mu, cov, cross, setup):
    Linv, zb, best, zq = setup
    A = cross @ Linv.T
    D = 0.5 * (cov + cov.transpose(1, 2)) - A @ A.transpose(1, 2)
    L = acqf.psd_safe_cholesky(D)
    f = mu.unsqueeze(0) + torch.einsum("bij,sj->sbi", A, zb) + torch.einsum("bij,sj->sbi", L, zq)
    if not acq._log:
        return torch.relu(f.amax(dim=-1) - best.unsqueeze(-1)).mean(dim=0)
    li = acqf.log_fatplus(f - best.view(-1, 1, 1), acq.tau_relu)
    return acqf.logmeanexp(acqf.fatmax(li, acq.tau_max), dim=0)


def shape(name, B, q, grad, log):
    acq = acqs[log]
    # q-batches around the baseline points, where samples improve
    near = Xb[torch.tensor(rng.integers(0, Xb.shape[0], B * q), device=dev)].reshape(B, q, a.d)
    Xq = (near + 0.05 * torch.tensor(rng.standard_normal((B, q, a.d)), device=dev)).clamp(0.0, 1.0)
    setup = acq._setup(q)
    nb = acq.X_baseline.shape[0]
    chunk = max(1, min(16384 // q, 2048 // q))  # gen_batch_initial_conditions' chunks

    def whole():
        if grad:
            Xg = Xq.clone().requires_grad_(True)
            torch.autograd.grad(acq(Xg).sum(), Xg)
        else:
            acqf._eval_batched(acq, Xq, chunk)

    def moments():
        if grad:
            Xg = Xq.clone().requires_grad_(True)
            mu, cov = acqf.posterior_moments(gp, Xg, obj)
            torch.autograd.grad(mu.sum() + cov.sum(), Xg)
        else:
            with torch.no_grad():
                for s in range(0, B, chunk):
                    acqf.posterior_moments(gp, Xq[s:s + chunk], obj)

    def cross(fn):
        if grad:
            Xg = Xq.reshape(B * q, a.d).clone().requires_grad_(True)
            torch.autograd.grad(fn(acq, Xg).sum(), Xg)
        else:
            with torch.no_grad():
                for s in range(0, B, chunk):
                    fn(acq, Xq[s:s + chunk].reshape(-1, a.d))

    with torch.no_grad():
        mu0, cov0 = acqf.posterior_moments(gp, Xq[:chunk], obj)
        cross0 = cross_gpx(acq, Xq[:chunk].reshape(-1, a.d)).reshape(-1, q, nb)
        dcross = float((cross_torch(acq, Xq[:chunk].reshape(-1, a.d)).reshape(-1, q, nb) - cross0).abs().max())
        v_gpx, v_torch = mc_gpx(acq, mu0, cov0, cross0, setup), mc_torch(acq, mu0, cov0, cross0, setup)
        dv = float((v_gpx - v_torch).abs().max())

    def mc(fn):
        if grad:
            leaves = tuple(x.clone().requires_grad_(True) for x in (mu0, cov0, cross0))
            torch.autograd.grad(fn(acq, *leaves, setup).sum(), leaves)
        else:
            with torch.no_grad():
                for s in range(0, B, chunk):
                    fn(acq, mu0, cov0, cross0, setup)

    work = {"whole": whole, "moments": moments, "cross_gpx": lambda: cross(cross_gpx),
            "cross_torch": lambda: cross(cross_torch), "mc_gpx": lambda: mc(mc_gpx), "mc_torch": lambda: mc(mc_torch)}
    for _ in range(a.warmup):
        for fn in work.values():
            fn()
    times = {k: [] for k in work}
    for _ in range(a.reps):  # the arms alternate
        for k, fn in work.items():
            times[k].append(timed(fn))
    rec = {"shape": name, "acq": "qlognei" if log else "qnei", "B": B, "q": q, "nb": nb, "S": a.samples, "n": a.n,
           "d": a.d, "grad": grad, "reps": a.reps, "cross_form": "valu", "improving_batches": int((v_gpx > 0).sum()) if
           not log else None, "max_cross_dev_vs_torch": dcross, "max_value_dev_vs_torch": dv}
    for k, ts in times.items():
        rec[k + "_ms"] = round(statistics.median(ts), 4)
        rec[k + "_min_ms"] = round(min(ts), 4)
    rec["cross_speedup"] = round(rec["cross_torch_ms"] / rec["cross_gpx_ms"], 2)
    rec["mc_speedup"] = round(rec["mc_torch_ms"] / rec["mc_gpx_ms"], 2)
    rec["torch_chain_ms"] = round(rec["moments_ms"] + rec["cross_torch_ms"] + rec["mc_torch_ms"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as fh:
            fh.write(line + "\n")


for log in (0, 1):
    shape("grad_B5_q4", 5, 4, True, log)
    shape("score_1024_q4", 1024, 4, False, log)
