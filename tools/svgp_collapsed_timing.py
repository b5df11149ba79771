"""Time of the closed-form SVGP variational posterior (default T = 8 tasks, M = 2048 inducing points, d = 5,
scale_linear_matern52, n in {10000, 100000}): GPEngine.svgp_fit_collapsed (gpx_svgp_fit_collapsed_f64) against the same
arithmetic written as a torch chain on the same GPU, which is what a user would otherwise write: kernel build,
cholesky, solve_triangular, matmul, cholesky, cholesky_inverse, per task.

    tools/svgp_collapsed_timing.py --ns 10000,100000 [--chunk C] [--out FILE]

runs every n as a step of its own: a fresh child process under `timeout`, the arms alternating inside it after --warmup
calls; the first step that fails or runs out of time ends the run.  A step prints one JSON line with

  gpx_ms / gpx_min_ms      median / minimum of --steps device-event timings of svgp_fit_collapsed
  torch_ms / torch_min_ms  the same of the torch chain
  gpx_peak / torch_peak    achieved fraction of the fp64 MFMA peak (--peak-tflops), counted on 2 M^2 n T flops at the median
  dmean / dcov             the two arms' q(u): max |m_gpx - m_torch| / max |m|, max |S_gpx - S_torch| / max |S|

--arms gpx times the library alone."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--ns", default="10000,100000", help="comma-separated training set sizes, one step each")
ap.add_argument("--M", type=int, default=2048)
ap.add_argument("--d", type=int, default=5)
ap.add_argument("--T", type=int, default=8)
ap.add_argument("--chunk", type=int, default=0, help="columns of X per pass (0: the library's default)")
ap.add_argument("--arms", default="gpx,torch")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--peak-tflops", type=float, default=78.6, help="fp64 MFMA peak of the device")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
a = ap.parse_args()

if a.child is None:
    # the driver never opens the GPU: one child per step, each under its own time limit, stop at the first failure
    for n in a.ns.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", n]
        for name in ("M", "d", "T", "chunk", "arms", "seed", "warmup", "steps", "peak_tflops"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
        if a.out:
            cmd += ["--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"step n={n} ended with status {rc}: stopping")
    sys.exit(0)

import math  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesianoptimizer_amd import GPEngine, KernelParams  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("svgp_collapsed_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
n, M, d, T = int(a.child), a.M, a.d, a.T
arms = a.arms.split(",")
JITTER = 1e-4

rng = np.random.default_rng(a.seed)
X = torch.tensor(0.6 * rng.standard_normal((n, d)), device=dev)
Z = X[torch.tensor(rng.choice(n, size=M, replace=False), device=dev)].unsqueeze(0).expand(T, -1, -1).contiguous()
params, Ycols = [], []
for t in range(T):
    ls, lv = 0.8 + rng.random(d), 0.05 + 0.1 * rng.random(d)
    params.append(KernelParams("scale_linear_matern52", list(ls), outputscale=0.5 + rng.random(), noise=1e-3 * (t + 1),
                               const_mean=0.1 * t - 0.2, linear_variance=list(lv)))
    w = torch.tensor(rng.standard_normal(d), device=dev)
    Ycols.append(torch.sin(X @ w) + 0.03 * torch.tensor(rng.standard_normal(n), device=dev))
Y = torch.stack(Ycols, dim=1).contiguous()
eng = GPEngine(0)


def kernel(A, B, p):
    """ScaleKernel(Linear + Matern-5/2) with ARD lengthscales and linear variances."""
    ls = torch.tensor(p.lengthscales(d), device=dev)
    lv = torch.tensor(p.linear_variances(d), device=dev)
    r = torch.cdist(A / ls, B / ls)
    s5r = math.sqrt(5.0) * r
    return p.outputscale * ((A * lv) @ B.T + (1.0 + s5r + (5.0 / 3.0) * r * r) * torch.exp(-s5r))


def torch_chain():
    ms, Ss = [], []
    eye = torch.eye(M, dtype=torch.float64, device=dev)
    for t, p in enumerate(params):
        L = torch.linalg.cholesky(kernel(Z[t], Z[t], p) + JITTER * eye)
        Phi = torch.linalg.solve_triangular(L, kernel(Z[t], X, p), upper=False)
        B = eye + (Phi @ Phi.T) / p.noise
        b = Phi @ (Y[:, t] - p.const_mean) / p.noise
        LB = torch.linalg.cholesky(B)
        Ss.append(torch.cholesky_inverse(LB))
        ms.append(torch.cholesky_solve(b.unsqueeze(-1), LB).squeeze(-1))
        del Phi, B
    return torch.stack(ms), torch.stack(Ss)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


work = {}
if "gpx" in arms:
    work["gpx"] = lambda: eng.svgp_fit_collapsed(params, Z, X, Y, jitter=JITTER, chunk=a.chunk or None)
if "torch" in arms:
    work["torch"] = torch_chain
for _ in range(a.warmup):
    for fn in work.values():
        fn()
times = {name: [] for name in work}
for _ in range(a.steps):
    for name, fn in work.items():
        times[name].append(timed(fn))
flops = 2.0 * M * M * n * T
rec = {"n": n, "M": M, "d": d, "T": T, "chunk": a.chunk, "steps": a.steps, "flops": flops}
for name, ts in times.items():
    rec[name + "_ms"] = round(statistics.median(ts), 3)
    rec[name + "_min_ms"] = round(min(ts), 3)
    rec[name + "_peak"] = round(flops / (statistics.median(ts) * 1e-3) / (a.peak_tflops * 1e12), 4)
if "gpx" in work and "torch" in work:
    vmean, vchol, _ = work["gpx"]()
    m_t, S_t = torch_chain()
    S_g = vchol @ vchol.transpose(1, 2)
    rec["dmean"] = float((vmean - m_t).abs().max() / m_t.abs().max())
    rec["dcov"] = float((S_g - S_t).abs().max() / S_t.abs().max())
    rec["speedup"] = round(rec["torch_ms"] / rec["gpx_ms"], 2)
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
