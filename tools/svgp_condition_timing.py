"""Time of conditioning the sparse model on new observations (default T = 8 tasks, M = 2048 inducing points, d = 5,
scale_linear_matern52, a model fitted on n = 100000 points): one GPEngine.svgp_condition (gpx_svgp_condition_f64) against
what reaches the same state without it, svgp_fit_collapsed on the n + n_new points followed by svgp_prepare.

    tools/svgp_condition_timing.py --configs 32,1024 [--out FILE]

runs every n_new as a step of its own: a fresh child process under `timeout`, the arms alternating inside it after
--warmup calls; the first step that fails or runs out of time ends the run.  A step prints one JSON line with

  condition_ms / condition_min_ms  median / minimum of --steps device-event timings of svgp_condition (with the
                                   variational pair, as SVGPPredictor.condition_on_observations calls it)
  refit_ms / refit_min_ms          the same of svgp_fit_collapsed(n + n_new) + svgp_prepare
  *_runs_min_ms                    per arm, the minimum of each of --runs consecutive thirds of the timings (the spread)
  ratio_min                        refit_min_ms / condition_min_ms
  repeat                           a second svgp_condition call returns the same bits
  dmu, dvar                        the conditioned predictive against the refit's at 4096 points, relative to max|mu|
                                   and max var

The call's split into projection, factor + inverse and compose comes from a kernel trace of `--arms condition` in a run
of its own (a profiler's kernel trace with statistics around this script); the timings above are taken without one."""
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
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--kernel", default="scale_linear_matern52")
ap.add_argument("--configs", default="32,1024", help="comma-separated n_new steps")
ap.add_argument("--arms", default="condition,refit")
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
        for name in ("M", "d", "T", "n", "kernel", "arms", "seed", "warmup", "steps", "runs"):
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
    sys.exit("svgp_condition_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
k = int(a.child)
arms = a.arms.split(",")

# standardised inputs N(0, 1), inducing points a random subset of them, outputs a smooth function plus noise
rng = np.random.default_rng(a.seed)
X = rng.standard_normal((a.n + k, a.d))
Z1 = X[rng.choice(a.n, size=a.M, replace=False)]
params, cols = [], []
for t in range(a.T):
    noise = 1e-3 * (1 + t)
    params.append(KernelParams(a.kernel, list(0.8 + rng.random(a.d)), outputscale=0.5 + 0.1 * t, noise=noise,
                               const_mean=0.1 * t - 0.2, linear_variance=list(0.05 + 0.1 * rng.random(a.d))))
    cols.append(np.sin(X @ rng.standard_normal(a.d)) + np.sqrt(noise) * rng.standard_normal(a.n + k))
Xd, Yd = torch.tensor(X, device=dev), torch.tensor(np.stack(cols, 1), device=dev)
Zd = torch.tensor(np.repeat(Z1[None], a.T, axis=0), device=dev)
eng = GPEngine(0)
vmean, vchol, _ = eng.svgp_fit_collapsed(params, Zd, Xd[:a.n], Yd[:a.n])
prep = eng.svgp_prepare(params, Zd, vmean, vchol, jitter=1e-4)
Xn, Yn = Xd[a.n:], Yd[a.n:]


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def refit():
    vm, vc, _ = eng.svgp_fit_collapsed(params, Zd, Xd, Yd)
    return eng.svgp_prepare(params, Zd, vm, vc, jitter=1e-4)


work = {}
if "condition" in arms:
    work["condition"] = lambda: eng.svgp_condition(prep, Xn, Yn, vmean=vmean, vchol=vchol)
if "refit" in arms:
    work["refit"] = refit
for _ in range(a.warmup):
    for fn in work.values():
        fn()
times = {name: [] for name in work}
for _ in range(a.steps):
    for name, fn in work.items():
        times[name].append(timed(fn))
rec = {"n_new": k, "n": a.n, "M": a.M, "d": a.d, "T": a.T, "kernel": a.kernel, "steps": a.steps}
if "condition" in work:
    p1, m1, c1 = work["condition"]()
    p2, m2, c2 = work["condition"]()
    bits = lambda u, v: bool(torch.equal(u.view(torch.int64), v.view(torch.int64)))  # noqa: E731
    rec["repeat"] = bits(p1["W2"], p2["W2"]) and bits(p1["alpha"], p2["alpha"]) and bits(m1, m2) and bits(c1, c2)
    if "refit" in work:
        Xq = torch.tensor(rng.standard_normal((4096, a.d)), device=dev)
        mu_c, var_c, _ = eng.svgp_predict(p1, Xq, want=("mean", "var"))
        mu_r, var_r, _ = eng.svgp_predict(work["refit"](), Xq, want=("mean", "var"))
        rec["dmu"] = float((mu_c - mu_r).abs().max() / mu_r.abs().max())
        rec["dvar"] = float((var_c - var_r).abs().max() / var_r.abs().max())
per = max(1, a.steps // a.runs)
for name, ts in times.items():
    rec[name + "_ms"] = round(statistics.median(ts), 4)
    rec[name + "_min_ms"] = round(min(ts), 4)
    rec[name + "_runs_min_ms"] = [round(min(ts[r * per:(r + 1) * per]), 4) for r in range(a.runs) if ts[r * per:(r + 1) * per]]
if "condition" in work and "refit" in work:
    rec["ratio_min"] = round(rec["refit_min_ms"] / rec["condition_min_ms"], 4)
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
