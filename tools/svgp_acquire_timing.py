"""Time of one analytic acquisition sweep on the sparse model (default T = 8 tasks, M = 2048 inducing points, d = 5,
scale_linear_matern52, 2^17 candidates, LogEI, k = 16): GPEngine.svgp_acquire (gpx_svgp_acquire_f64) against
svgp_predict(want=("score",)) followed by gpx_topk_f64 on the same handle and prepared model.  That composition is the
same K* builds and products with the predictive's finalize in place of the objective's, so it is what the new call
should cost; its scores are the variance sum, not an acquisition, and the results are not compared.

    tools/svgp_acquire_timing.py --configs logei:16,ucb:16,logei:1024 [--out FILE]

runs every ACQ:K configuration as a step of its own: a fresh child process under `timeout`, the arms alternating inside
it after --warmup calls; the first step that fails or runs out of time ends the run.  A step prints one JSON line with

  acquire_ms / acquire_min_ms    median / minimum of --steps device-event timings of svgp_acquire
  composed_ms / composed_min_ms  the same of svgp_predict(want=("score",)) + topk
  *_runs_min_ms                  per arm, the minimum of each of --runs consecutive thirds of the timings (the spread)
  ratio_min                      acquire_min_ms / composed_min_ms
  repeat                         a second svgp_acquire call returns the same bits"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=2048)
ap.add_argument("--d", type=int, default=5)
ap.add_argument("--T", type=int, default=8)
ap.add_argument("--m", type=int, default=1 << 17)
ap.add_argument("--kernel", default="scale_linear_matern52")
ap.add_argument("--configs", default="logei:16", help="comma-separated ACQ:K steps")
ap.add_argument("--arms", default="acquire,composed")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=9)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
a = ap.parse_args()

if a.child is None:
    # the driver never opens the GPU: one child per step, each under its own time limit, stop at the first failure
    for cfg in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", cfg]
        for name in ("M", "d", "T", "m", "kernel", "arms", "seed", "warmup", "steps", "runs"):
            cmd += ["--" + name, str(getattr(a, name))]
        if a.out:
            cmd += ["--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"step {cfg} ended with status {rc}: stopping")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesianoptimizer_amd import GPEngine, KernelParams  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("svgp_acquire_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
acq, k = a.child.split(":")
k = int(k)
arms = a.arms.split(",")

# a trained model's shape, not its values: inducing points and candidates N(0, 1) (standardised inputs), a random
# variational mean and a well-conditioned lower-triangular factor
rng = np.random.default_rng(a.seed)
Z = rng.standard_normal((a.T, a.M, a.d))
vmean = rng.standard_normal((a.T, a.M))
vchol = np.tril(0.3 * rng.standard_normal((a.T, a.M, a.M)) / np.sqrt(a.M), -1) + 0.5 * np.eye(a.M)
params = [KernelParams(a.kernel, list(0.8 + rng.random(a.d)), outputscale=0.5 + 0.1 * t, noise=1e-3 * (1 + t),
                       const_mean=0.1 * t - 0.2, linear_variance=list(0.05 + 0.1 * rng.random(a.d))) for t in range(a.T)]
eng = GPEngine(0)
prep = eng.svgp_prepare(params, torch.tensor(Z, device=dev), torch.tensor(vmean, device=dev),
                        torch.tensor(vchol, device=dev), jitter=1e-4)
Xs = torch.tensor(rng.standard_normal((a.m, a.d)), device=dev)
kw = dict(best_f=0.5, beta=4.0, weights=[1.0 / a.T] * a.T)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def composed():
    _, _, sc = eng.svgp_predict(prep, Xs, want=("score",))
    return eng.topk(sc, k)


work = {}
if "acquire" in arms:
    work["acquire"] = lambda: eng.svgp_acquire(prep, Xs, k, acq, **kw)
if "composed" in arms:
    work["composed"] = composed
for _ in range(a.warmup):
    for fn in work.values():
        fn()
times = {name: [] for name in work}
for _ in range(a.steps):
    for name, fn in work.items():
        times[name].append(timed(fn))
rec = {"acq": acq, "k": k, "M": a.M, "d": a.d, "T": a.T, "m": a.m, "kernel": a.kernel, "steps": a.steps}
if "acquire" in work:
    v, i = work["acquire"]()
    v2, i2 = work["acquire"]()
    rec["repeat"] = bool(torch.equal(v.view(torch.int64), v2.view(torch.int64)) and torch.equal(i, i2))
    rec["best"] = [float(v[0]), int(i[0])]
per = max(1, a.steps // a.runs)
for name, ts in times.items():
    rec[name + "_ms"] = round(statistics.median(ts), 4)
    rec[name + "_min_ms"] = round(min(ts), 4)
    rec[name + "_runs_min_ms"] = [round(min(ts[r * per:(r + 1) * per]), 4) for r in range(a.runs) if ts[r * per:(r + 1) * per]]
if "acquire" in work and "composed" in work:
    rec["ratio_min"] = round(rec["acquire_min_ms"] / rec["composed_min_ms"], 4)
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
