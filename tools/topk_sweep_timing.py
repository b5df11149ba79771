"""Time of the k best candidates of one acquisition sweep on the bench problem (default n = 4096, d = 8, RBF, logEI,
2^20 Sobol candidates, bench.py's data): GPEngine.acquire_topk (gpx_acquire_topk_f64, the pruned sweep with the k-th
best exact score as its incumbent) against the composition it replaces, the full sweep with scores followed by
gpx_topk_f64, on the same handle and fit.  Per k it prints one JSON line with

  topk_ms         median time of acquire_topk
  composed_ms     median time of acquire(return_scores=True) + topk
  sweep_stats     gpx_sweep_stats after an acquire_topk call
  equal           the two results have the same bits

and for k = 1 the cost of the per-round pool launches: topk_ms minus the median time of engine.acquire (the argmax
form of the same pruned sweep) in the same process.  Every figure is the median of --steps device-event timings after
--warmup calls; the arms alternate."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--d", type=int, default=8)
ap.add_argument("--m", type=int, default=1 << 20)
ap.add_argument("--kernel", default="rbf")
ap.add_argument("--acq", default="logei")
ap.add_argument("--ks", default="1,16,64,1024")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("topk_sweep_timing needs a ROCm device: a CPU run gives no timing")
dev = torch.device("cuda", 0)

X_np, y_np = synthetic.problem(a.n, a.d, a.seed)
Xs = torch.tensor(synthetic.sobol(a.m, a.d, a.seed + 1), device=dev)
eng = GPEngine(0)
st = eng.fit(torch.tensor(X_np, device=dev), torch.tensor(y_np, device=dev),
             KernelParams(a.kernel, botorch_default_lengthscale(a.d), noise=1e-4))
kw = dict(best_f=float(y_np.max()), beta=4.0)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def composed(k):
    _, _, sc = eng.acquire(st, Xs, a.acq, return_scores=True, **kw)
    return eng.topk(sc, k)


for k in [int(v) for v in a.ks.split(",")]:
    work = {"topk": lambda: eng.acquire_topk(st, Xs, k, a.acq, **kw), "composed": lambda: composed(k)}
    if k == 1:
        work["argmax"] = lambda: eng.acquire(st, Xs, a.acq, **kw)
    for _ in range(a.warmup):
        for fn in work.values():
            fn()
    times = {name: [] for name in work}
    for _ in range(a.steps):
        for name, fn in work.items():
            times[name].append(timed(fn))
    v, i = eng.acquire_topk(st, Xs, k, a.acq, **kw)
    stats = eng.sweep_stats()
    vr, ir = composed(k)
    rec = {"k": k, "n": a.n, "d": a.d, "m": a.m, "kernel": a.kernel, "acq": a.acq, "steps": a.steps,
           "sweep_stats": list(stats),
           "equal": bool(torch.equal(v.view(torch.int64), vr.view(torch.int64)) and torch.equal(i, ir))}
    for name, ts in times.items():
        rec[name + "_ms"] = round(statistics.median(ts), 4)
        rec[name + "_min_ms"] = round(min(ts), 4)
    rec["speedup"] = round(rec["composed_ms"] / rec["topk_ms"], 2)
    if k == 1:
        rec["pool_launches_ms"] = round(rec["topk_ms"] - rec["argmax_ms"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as fh:
            fh.write(line + "\n")
