"""Sweep-only timings of the pruned acquisition sweep (2^20 candidates, d = 8, RBF, logEI), one JSON line per case:
[ms of each repetition], sweep_stats, (best value, best index), [host wall ms of each repetition: the call followed by
a device synchronise, which also sees a wait inside the call that device events do not].  Cases: 2^20 identical
candidates at n = 4096 (nothing prunable) with sweep_prune 0 / 1, the bench problem (seed 0), the seed-1000 problem, and padded n = 384 .. 2048 with
sweep_prune 0 / 2.  The library is the tree's, or GPX_LIB's (A/B runs alternate processes)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cases", default="worst,bench,hard,small")
ap.add_argument("--tag", default="")
a = ap.parse_args()
D, M = 8, 1 << 20
dev = torch.device("cuda", 0)
eng = GPEngine(0)
kp = KernelParams("rbf", botorch_default_lengthscale(D), noise=1e-4)


def run(name, st, Xs, best_f, opt):
    eng.set_option("sweep_prune", opt)
    eng.acquire(st, Xs, "logei", best_f=best_f)  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        bv, bi = eng.acquire(st, Xs, "logei", best_f=best_f)
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(e0.elapsed_time(e1))
    print(json.dumps([f"{a.tag}{name}_opt{opt}", ms, list(eng.sweep_stats()), [float(bv.item()), int(bi.item())],
                      wall]), flush=True)


def problem(n, seed):
    X, y = synthetic.problem(n, D, seed)
    st = eng.fit(torch.tensor(X, device=dev), torch.tensor(y, device=dev), kp)
    return st, float(y.max())


cases = a.cases.split(",")
if "worst" in cases or "bench" in cases:
    st, bf = problem(4096, 0)
    Xs = torch.tensor(synthetic.sobol(M, D, 1), device=dev)
    if "worst" in cases:
        same = Xs[17:18].repeat(M, 1).contiguous()
        for opt in (0, 1):
            run("worst_n4096", st, same, bf, opt)
        del same
    if "bench" in cases:
        for opt in (0, 1):
            run("bench_problem_seed0", st, Xs, bf, opt)
if "hard" in cases:
    st, bf = problem(4096, 1000)
    Xs = torch.tensor(synthetic.sobol(M, D, 1001), device=dev)
    for opt in (0, 1):
        run("hard_problem_seed1000", st, Xs, bf, opt)
if "small" in cases:
    Xs = torch.tensor(synthetic.sobol(M, D, 1), device=dev)
    for n in (384, 640, 1024, 2048):
        st, bf = problem(n, 0)
        for opt in (0, 2):
            run(f"n{n}", st, Xs, bf, opt)
