"""Time of one evaluation of the collapsed SVGP bound and its hyperparameter gradient (default T = 8 tasks, M = 2048
inducing points, d = 5, scale_linear_matern52; n = 10,000 and 100,000), up to four arms on the same GPU and data:

  grad      GPEngine.svgp_bound_grad (gpx_svgp_bound_grad_f64): the fit's pass over X and the gradient's second pass
  gradz     GPEngine.svgp_bound_grad_z (gpx_svgp_bound_grad_z_f64): the same with the inducing locations' gradient
            (not in the default arms: --arms grad,gradz,fit gives gradz_over_grad and gradz_over_fit)
  fit       GPEngine.svgp_fit_collapsed (gpx_svgp_fit_collapsed_f64) alone
  autograd  the same value and gradient by torch autograd on the device, task after task (K(Z, X) and the graph of
            one task are all it holds at a time); its gradient is compared with the grad arm's

    tools/svgp_grad_timing.py --ns 10000,100000 [--out FILE]

runs every n as a step of its own: a fresh child process under `timeout`, the arms alternating inside it after --warmup
calls; the first step that fails or runs out of time ends the run.  A step prints one JSON line with, per arm, the median
and the minimum of --steps device-event timings (ms), grad_over_fit = grad_min_ms / fit_min_ms (the second pass repeats
the first's 2 M^2 n MFMA flops per task, so about 2 is the figure to explain), the fp64 flop rate of the two passes'
products in the grad arm, and the largest entrywise disagreement of the two gradients relative to the largest entry."""
import argparse
import json
import math
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
ap.add_argument("--kernel", default="scale_linear_matern52")
ap.add_argument("--arms", default="grad,fit,autograd")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=400, help="seconds a step may take")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
a = ap.parse_args()

if a.child is None:
    # the driver never opens the GPU: one child per step, each under its own time limit, stop at the first failure
    for n in a.ns.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", n]
        for name in ("M", "d", "T", "kernel", "arms", "seed", "warmup", "steps"):
            cmd += ["--" + name, str(getattr(a, name))]
        if a.out:
            cmd += ["--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"step n={n} ended with status {rc}: stopping")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesianoptimizer_amd import GPEngine, KernelParams, _capi  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("svgp_grad_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
n, M, d, T = int(a.child), a.M, a.d, a.T
arms = a.arms.split(",")
JITTER = 1e-4

rng = np.random.default_rng(a.seed)
X_np = 0.6 * rng.standard_normal((n, d))
Z_np = X_np[rng.choice(n, size=M, replace=False)]
Y_np = np.stack([np.sin(X_np @ rng.standard_normal(d)) + 0.3 * (X_np @ rng.standard_normal(d))
                 + 0.05 * rng.standard_normal(n) for _ in range(T)], axis=1)
params = [KernelParams(a.kernel, list(0.8 + rng.random(d)), outputscale=0.5 + rng.random(), noise=1e-2 * (1 + t),
                       const_mean=0.1 * t - 0.2, linear_variance=list(0.05 + 0.1 * rng.random(d))) for t in range(T)]
X, Y = torch.tensor(X_np, device=dev), torch.tensor(Y_np, device=dev)
Z = torch.tensor(Z_np, device=dev).unsqueeze(0).expand(T, -1, -1).contiguous()
eng = GPEngine(0)
SQRT5 = math.sqrt(5.0)


def kernel_t(A, B, ls, os_, lv):
    """k(A, B) in GPyTorch's expanded distance form (one matmul), differentiable."""
    As, Bs = A / ls, B / ls
    r2 = ((As * As).sum(1)[:, None] + (Bs * Bs).sum(1)[None, :] - 2.0 * As @ Bs.T).clamp_min(0.0)
    if a.kernel == "rbf":
        return os_ * torch.exp(-0.5 * r2)
    r = torch.sqrt(r2 + 1e-30)
    mat = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-SQRT5 * r)
    return os_ * (mat + (A * lv) @ B.T) if a.kernel == "scale_linear_matern52" else os_ * mat


def autograd():
    out = []
    for t, p in enumerate(params):
        th = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True)
              for v in (p.noise, p.outputscale, p.const_mean, p.lengthscales(d), p.linear_variances(d))]
        s2, os_, c, ls, lv = th
        L = torch.linalg.cholesky(kernel_t(Z[t], Z[t], ls, os_, lv) + JITTER * torch.eye(M, dtype=torch.float64,
                                                                                          device=dev))
        Phi = torch.linalg.solve_triangular(L, kernel_t(Z[t], X, ls, os_, lv), upper=False)
        r = Y[:, t] - c
        LB = torch.linalg.cholesky(torch.eye(M, dtype=torch.float64, device=dev) + Phi @ Phi.T / s2)
        u = torch.linalg.solve_triangular(LB, (Phi @ r / s2)[:, None], upper=False)[:, 0]
        kd = os_ * ((X * X * lv).sum(1) + 1.0) if a.kernel == "scale_linear_matern52" else os_ * n
        F = (-0.5 * n * torch.log(2.0 * math.pi * s2) - torch.log(torch.diagonal(LB)).sum() - 0.5 * (r @ r) / s2
             + 0.5 * (u @ u) - 0.5 * (kd.sum() - (Phi * Phi).sum()) / s2)
        g = torch.autograd.grad(-F, th, allow_unused=True)
        out.append(torch.cat([torch.zeros(d, dtype=torch.float64, device=dev) if v is None else v.reshape(-1)
                              for v in g]))
    return torch.stack(out)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


work = {}
if "grad" in arms:
    work["grad"] = lambda: eng.svgp_bound_grad(params, Z, X, Y, jitter=JITTER)
if "gradz" in arms:
    work["gradz"] = lambda: eng.svgp_bound_grad_z(params, Z, X, Y, jitter=JITTER)
if "fit" in arms:
    work["fit"] = lambda: eng.svgp_fit_collapsed(params, Z, X, Y, jitter=JITTER)
if "autograd" in arms:
    work["autograd"] = autograd
for _ in range(a.warmup):
    for fn in work.values():
        fn()
times = {name: [] for name in work}
for _ in range(a.steps):
    for name, fn in work.items():
        times[name].append(timed(fn))
rec = {"n": n, "M": M, "d": d, "T": T, "kernel": a.kernel, "steps": a.steps}
for name, ts in times.items():
    rec[name + "_ms"] = round(statistics.median(ts), 3)
    rec[name + "_min_ms"] = round(min(ts), 3)
if "gradz" in work:
    for other in ("grad", "fit"):
        if other in work:
            rec["gradz_over_" + other] = round(rec["gradz_min_ms"] / rec[other + "_min_ms"], 3)
if "grad" in work:
    Mpad = -(-M // _capi.GPX_TILE) * _capi.GPX_TILE
    # projection (triangular: half), rank update (lower tiles: half) and the second pass's full product, per task
    flops = T * (Mpad * Mpad * n + Mpad * Mpad * n + 2.0 * Mpad * Mpad * n)
    rec["grad_pass_tflops"] = round(flops / (rec["grad_min_ms"] * 1e-3) / 1e12, 2)
    if "fit" in work:
        rec["grad_over_fit"] = round(rec["grad_min_ms"] / rec["fit_min_ms"], 3)
    if "autograd" in work:
        rec["autograd_over_grad"] = round(rec["autograd_min_ms"] / rec["grad_min_ms"], 2)
        out, info = eng.svgp_bound_grad(params, Z, X, Y, jitter=JITTER)
        g = out[:, _capi.SVGP_GRAD_MLL:]
        mine = torch.cat([g[:, [_capi.MLL_D_NOISE, _capi.MLL_D_OUTPUTSCALE, _capi.MLL_D_MEAN]],
                          g[:, _capi.MLL_D_LENGTHSCALE:_capi.MLL_D_LENGTHSCALE + d],
                          g[:, _capi.MLL_D_LINVAR:_capi.MLL_D_LINVAR + d]], dim=1)
        ref = autograd()
        rec["info"] = info.cpu().tolist()
        rec["max_rel_to_largest_entry"] = float(((mine - ref).abs().amax(1) / ref.abs().amax(1)).max())
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
