"""Time of the k best candidates of one multi-output acquisition sweep (default n = 4096, d = 8, T = 8 outputs,
scale_linear_matern52, 2^17 Sobol candidates, LogEI, k = 16): GPEngine.acquire_topk_multi (gpx_acquire_topk_multi_f64,
the pruned sweep over independent outputs) against the composition it replaces, acquire_multi(return_scores=True)
followed by gpx_topk_f64, on the same handle and fits.

    tools/topk_multi_timing.py --configs logei:16,variance:16,logei:300 [--out FILE]

runs every ACQ:K configuration as a step of its own: a fresh child process under `timeout`, the arms alternating inside
it after --warmup calls; the first step that fails or runs out of time ends the run.  A step prints one JSON line with

  topk_ms / topk_min_ms          median / minimum of --steps device-event timings of acquire_topk_multi
  composed_ms / composed_min_ms  the same of acquire_multi(return_scores=True) + topk
  runs_min_ms                    per arm, the minimum of each of --runs consecutive thirds of the timings
  sweep_stats                    gpx_sweep_stats after an acquire_topk_multi call
  equal                          the two results have the same bits

--arms composed times the composition alone (a build without the entry point)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--T", type=int, default=8)
ap.add_argument("--m", type=int, default=1 << 17)
ap.add_argument("--kernel", default="scale_linear_matern52")
ap.add_argument("--configs", default="logei:16", help="comma-separated ACQ:K steps")
ap.add_argument("--arms", default="topk,composed")
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
        for name in ("n", "d", "T", "m", "kernel", "arms", "seed", "warmup", "steps", "runs"):
            cmd += ["--" + name, str(getattr(a, name))]
        if a.out:
            cmd += ["--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"step {cfg} ended with status {rc}: stopping")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, synthetic  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("topk_multi_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
acq, k = a.child.split(":")
k = int(k)
arms = a.arms.split(",")

X_np, y0 = synthetic.problem(a.n, a.d, a.seed)
rng = np.random.default_rng(a.seed + 5)
cols = [y0] + [np.cos(4.0 * X_np @ rng.random(a.d) + t) + 0.3 * y0 for t in range(1, a.T)]
Y_np = np.stack([(c - c.mean()) / c.std() for c in cols], axis=1)
params = [KernelParams(a.kernel, botorch_default_lengthscale(a.d) * (0.8 + 0.05 * t), outputscale=1.0 + 0.1 * t,
                       noise=1e-4 * (1 + t), const_mean=0.05 * t, linear_variance=0.3) for t in range(a.T)]
Xs = torch.tensor(synthetic.sobol(a.m, a.d, a.seed + 1), device=dev)
eng = GPEngine(0)
states = eng.fit_outputs(torch.tensor(X_np, device=dev), torch.tensor(Y_np, device=dev), params)
w = [1.0 / a.T] * a.T
kw = dict(best_f=float((Y_np @ np.array(w)).max()), beta=4.0, weights=w)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def composed():
    _, _, sc = eng.acquire_multi(states, Xs, acq, return_scores=True, **kw)
    return eng.topk(sc, k)


work = {}
if "topk" in arms:
    work["topk"] = lambda: eng.acquire_topk_multi(states, Xs, k, acq, **kw)
if "composed" in arms:
    work["composed"] = composed
for _ in range(a.warmup):
    for fn in work.values():
        fn()
times = {name: [] for name in work}
for _ in range(a.steps):
    for name, fn in work.items():
        times[name].append(timed(fn))
rec = {"acq": acq, "k": k, "n": a.n, "d": a.d, "T": a.T, "m": a.m, "kernel": a.kernel, "steps": a.steps}
if "topk" in work:
    v, i = eng.acquire_topk_multi(states, Xs, k, acq, **kw)
    rec["sweep_stats"] = list(eng.sweep_stats())
    if "composed" in work:
        vr, ir = composed()
        rec["equal"] = bool(torch.equal(v.view(torch.int64), vr.view(torch.int64)) and torch.equal(i, ir))
per = max(1, a.steps // a.runs)
for name, ts in times.items():
    rec[name + "_ms"] = round(statistics.median(ts), 4)
    rec[name + "_min_ms"] = round(min(ts), 4)
    rec[name + "_runs_min_ms"] = [round(min(ts[r * per:(r + 1) * per]), 4) for r in range(a.runs) if ts[r * per:(r + 1) * per]]
if "topk" in work and "composed" in work:
    rec["speedup_min"] = round(rec["composed_min_ms"] / rec["topk_min_ms"], 2)
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
