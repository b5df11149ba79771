"""Time of the sparse model's q-batch moments (gpx_svgp_moments_grad_f64) against the same formulas as a torch chain with
autograd, on the same GPU and from the same prepared model (T = 1, default M = 2048 inducing points of n = 8192, d = 5,
ScaleKernel(Linear + Matern-5/2)):

  grad_B5_q4     one L-BFGS-B evaluation of optimize_acqf: the moments of B = 5 restarts x q = 4 candidates and the
                 gradient of a fixed linear function of them w.r.t. the candidates.  ``call``: the library call alone
                 (it returns the derivatives); ``lib``: acqf._Moments, the call and its chain rule; ``torch``: V = W^T K*,
                 U = W2^T K*, mean and covariance in torch from the same W, W2 and alpha', backward by autograd.
  value_1024_q4  raw-sample scoring: mean and covariance of 1024 x 4 candidates, no derivatives.  ``lib``: the value-only
                 call; ``torch``: the chain under no_grad.

The arms alternate in one process; every figure is the median of --reps device-event timings after --warmup evaluations.
The largest deviation between the two arms' results is reported beside the times.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bayesianoptimizer_amd import GPEngine, KernelParams, acqf
from bayesianoptimizer_amd.engine import SVGPTaskState
from bayesianoptimizer_amd.svgp import SVGPModel

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=2048)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--d", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None, help="also append the JSON line to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("svgp_moments_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)
eng = GPEngine(0)
rng = np.random.default_rng(0)
M, d = a.M, a.d

X = torch.tensor(rng.random((a.n, d)), device=dev)
y = torch.sin(3.0 * X[:, 0]) + (X[:, 1:] ** 2).sum(1) + 0.05 * torch.randn(a.n, dtype=torch.float64, device=dev)
ls = [0.6 + 0.1 * k for k in range(d)]
lv = [0.05 + 0.05 * k for k in range(d)]
kp = KernelParams("scale_linear_matern52", ls, outputscale=1.2, noise=1e-2, const_mean=0.1, linear_variance=lv)
Z = X[torch.as_tensor(rng.permutation(a.n)[:M], device=dev)]
model = SVGPModel.fit_collapsed(X, y.unsqueeze(-1), kp, Z, engine=eng)
prep = eng.svgp_prepare(model.params, model.Z, model.vmean, model.vchol, jitter=model.jitter)
state = SVGPTaskState(prep, 0, d, kp)
Zt, W, W2, alpha = prep["Z"][0], prep["W"][0][:M, :M], prep["W2"][0][:M, :M], prep["alpha"][0][:M]
t_ls = torch.tensor(ls, device=dev)
t_lv = torch.tensor(lv, device=dev)


def kernel(A, B):
    diff = (A.unsqueeze(-2) - B.unsqueeze(-3)) / t_ls
    r2 = (diff * diff).sum(-1)
    r = torch.sqrt(torch.where(r2 > 0, r2, torch.ones_like(r2))) * (r2 > 0)  # (no derivative of sqrt at 0)
    s5r = math.sqrt(5.0) * r
    return kp.outputscale * ((A * t_lv) @ B.transpose(-1, -2) + (1.0 + s5r + (5.0 / 3.0) * r2) * torch.exp(-s5r))


def torch_moments(Xq):
    """mean (B, q), cov (B, q, q) from the prepared W, W2, alpha'"""
    B, q, _ = Xq.shape
    Ks = kernel(Zt, Xq.reshape(B * q, d))  # (M, B q)
    V = (W.T @ Ks).reshape(M, B, q)
    U = (W2.T @ Ks).reshape(M, B, q)
    mean = kp.const_mean + (alpha @ Ks).reshape(B, q)
    cov = kernel(Xq, Xq) - torch.einsum("mbi,mbj->bij", V, V) + torch.einsum("mbi,mbj->bij", U, U)
    return mean, cov


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def measure(work):
    for _ in range(a.warmup):
        for fn in work.values():
            fn()
    times = {k: [] for k in work}
    for _ in range(a.reps):  # the arms alternate
        for k, fn in work.items():
            times[k].append(timed(fn))
    return {k: (round(statistics.median(ts), 4), round(min(ts), 4)) for k, ts in times.items()}


rec = {"M": M, "n": a.n, "d": d, "kind": kp.kind, "reps": a.reps, "warmup": a.warmup}

# ---- one gradient evaluation ---------------------------------------------------------------------------------------
B, q = 5, 4
Xg = torch.tensor(rng.random((B, q, d)), device=dev)
wm = torch.tensor(rng.standard_normal((B, q)), device=dev)
wc = torch.tensor(rng.standard_normal((B, q, q)), device=dev)


def grad_lib():
    Xr = Xg.clone().requires_grad_(True)
    mean, cov = acqf._Moments.apply(Xr.reshape(B * q, d), eng, state, q, state.alpha)
    return torch.autograd.grad((wm * mean.reshape(B, q)).sum() + (wc * cov.reshape(B, q, q)).sum(), Xr)[0]


def grad_torch():
    Xr = Xg.clone().requires_grad_(True)
    mean, cov = torch_moments(Xr)
    return torch.autograd.grad((wm * mean).sum() + (wc * cov).sum(), Xr)[0]


g_lib, g_torch = grad_lib(), grad_torch()
rec["grad_max_dev_rel"] = float((g_lib - g_torch).abs().max() / g_torch.abs().max())
res = measure({"call": lambda: eng.svgp_moments_grad(prep, 0, Xg.reshape(B * q, d), q), "lib": grad_lib,
               "torch": grad_torch})
for k, (med, low) in res.items():
    rec[f"grad_B5_q4_{k}_ms"], rec[f"grad_B5_q4_{k}_min_ms"] = med, low

# ---- value-only scoring --------------------------------------------------------------------------------------------
Bv = 1024
Xv = torch.tensor(rng.random((Bv, q, d)), device=dev)


def value_lib():
    return eng.svgp_moments_grad(prep, 0, Xv.reshape(Bv * q, d), q, need_grad=False)


def value_torch():
    with torch.no_grad():
        return torch_moments(Xv)


ml, _, cl, _ = value_lib()
mt, ct = value_torch()
rec["value_mean_max_dev_rel"] = float((ml.reshape(Bv, q) - mt).abs().max() / mt.abs().max())
rec["value_cov_max_dev"] = float((cl.reshape(Bv, q, q) - ct).abs().max())
res = measure({"lib": value_lib, "torch": value_torch})
for k, (med, low) in res.items():
    rec[f"value_1024_q4_{k}_ms"], rec[f"value_1024_q4_{k}_min_ms"] = med, low

line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "a", encoding="utf-8") as fh:
        fh.write(line + "\n")
