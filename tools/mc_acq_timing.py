"""Time of one acquisition evaluation of optimize_acqf with the Monte-Carlo part in torch (fused=False: batched
cholesky_ex with its host read, einsum, softplus / logsumexp chains, autograd backward) against gpx_mc_acq_f64
(fused=True), on a fitted exact GP (default n = 1024, d = 8, S = 512 base samples):

  grad_B5_q4    acq(X) and d/dX at B = 5 (batch_limit) q-batches of q = 4: one L-BFGS-B evaluation
  grad_B5_q1    the same at q = 1
  score_1024_q4 value-only scoring of 1024 raw q-batches of q = 4 (gen_batch_initial_conditions)

Each shape is split into the posterior-moments call (gpx_moments_grad_f64 and its chain rule, shared by both arms) and
the Monte-Carlo part alone on precomputed moments.  Both arms alternate in one process; every figure is the median of
--reps device-event timings (the events bracket the whole evaluation, host gaps and the unfused arm's synchronisation
included) after --warmup evaluations.  Prints one JSON line per shape and arm."""
import argparse
import json
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
ap.add_argument("--samples", type=int, default=512)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mc_acq_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)

X, y = synthetic.problem(a.n, a.d, seed=0)
gp = ExactGP(X, y.reshape(-1, 1), KernelParams("matern52", 0.5, noise=1e-3), outcome_transform=Standardize()).fit()
best_f = float(np.max(y))
arms = {fused: acqf.qLogExpectedImprovement(gp, best_f=best_f, fused=fused,
                                            sampler=acqf.SobolQMCNormalSampler(torch.Size([a.samples]), 11))
        for fused in (False, True)}
obj = arms[False].objective
rng = np.random.default_rng(1)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def mc_part(acq, mu, cov, z, grad):
    if acq.fused:
        opts = {"best_f": acq.best_f, "fat_relu": acq.fat, "fat_max": acq.fat_max, "tau_max": acq.tau_max,
                "tau_relu": acq.tau_relu}
        v = acqf._McAcq.apply(mu, cov, gp.engine, z, "qlogei", opts)
    else:
        v = acqf.qlogei_from_moments(mu, cov, z, acq.best_f, acq.fat, acq.tau_max, acq.tau_relu)
    if grad:
        torch.autograd.grad(v.sum(), (mu, cov))
    return v


def shape(name, B, q, grad):
    Xq = torch.tensor(rng.random((B, q, a.d)), device=dev)
    z = arms[False].sampler.base_samples(q, dev)
    chunk = max(1, min(16384 // q, 2048 // q))  # gen_batch_initial_conditions' chunks

    def whole(acq):
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

    with torch.no_grad():
        mu0, cov0 = acqf.posterior_moments(gp, Xq[:chunk], obj)

    def mc(acq):
        if grad:
            mc_part(acq, mu0.clone().requires_grad_(True), cov0.clone().requires_grad_(True), z, True)
        else:
            with torch.no_grad():
                for s in range(0, B, chunk):
                    mc_part(acq, mu0, cov0, z, False)

    with torch.no_grad():
        dv = float((arms[True](Xq[:chunk]) - arms[False](Xq[:chunk])).abs().max())
    work = {"moments": moments}
    for fused in (False, True):
        work[f"whole_fused{int(fused)}"] = lambda acq=arms[fused]: whole(acq)
        work[f"mc_fused{int(fused)}"] = lambda acq=arms[fused]: mc(acq)
    for _ in range(a.warmup):
        for fn in work.values():
            fn()
    times = {k: [] for k in work}
    for _ in range(a.reps):  # the arms alternate
        for k, fn in work.items():
            times[k].append(timed(fn))
    rec = {"shape": name, "B": B, "q": q, "S": a.samples, "n": a.n, "d": a.d, "grad": grad, "reps": a.reps,
           "max_value_dev_fused_vs_unfused": dv}
    for k, ts in times.items():
        rec[k + "_ms"] = round(statistics.median(ts), 4)
        rec[k + "_min_ms"] = round(min(ts), 4)
    rec["mc_speedup"] = round(rec["mc_fused0_ms"] / rec["mc_fused1_ms"], 2)
    rec["whole_speedup"] = round(rec["whole_fused0_ms"] / rec["whole_fused1_ms"], 2)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as fh:
            fh.write(line + "\n")


shape("grad_B5_q4", 5, 4, True)
shape("grad_B5_q1", 5, 1, True)
shape("score_1024_q4", 1024, 4, False)
