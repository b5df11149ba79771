#!/usr/bin/env python3
"""The launch sequence of the acquisition sweep's paths, for comparing two builds of libgpx.so.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/sweep_launch_trace.py run
    python3 tools/sweep_launch_trace.py seq OUT/..._kernel_trace.csv > NEW.txt
    python3 tools/sweep_launch_trace.py diff OLD.txt NEW.txt

`run` makes one call per path at n = 384 (three row tiles), m = 3000: the lazy pruned sweep (RBF d = 8, with the mean
bound; Matern d = 3, without), the chunked pruned sweep (d = 20), the top-k form (k = 16), the multi-output sweep
(T = 2), and the fused sweep at n = 200; it prints each result's bits.  Run it under a kernel trace (no counters) once
per library (GPX_LIB selects one other than the tree's).  `seq` prints the (kernel name, grid, workgroup) sequence of
the library's kernels in such a trace, one launch per line; `diff` compares two of them (either form); exit status 0:
identical.
"""
import csv
import difflib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import numpy as np
    import torch

    from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale
    from oracle import gp_oracle as O

    dev = torch.device("cuda", 0)
    eng = GPEngine(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)
    bits = lambda x: [int(v) for v in x.reshape(-1).view(torch.int64).tolist()]
    m, out = 3000, {}

    def problem(n, d, kind):
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams(kind, botorch_default_lengthscale(d), linear_variance=0.3, noise=1e-4)
        return X, y, kp, t(O.sobol_candidates(m, d, 22))

    for name, n, d, kind in (("lazy_rbf_d8", 384, 8, "rbf"), ("lazy_matern_d3", 384, 3, "matern52"),
                             ("chunked_pruned_d20", 384, 20, "matern52"), ("fused_n200", 200, 4, "rbf")):
        X, y, kp, Xs = problem(n, d, kind)
        st = eng.fit(t(X), t(y), kp)
        bv, bi = eng.acquire(st, Xs, "logei", best_f=float(y.max()))
        out[name] = bits(bv) + bits(bi) + list(eng.sweep_stats())
    X, y, kp, Xs = problem(384, 8, "rbf")
    st = eng.fit(t(X), t(y), kp)
    val, idx = eng.acquire_topk(st, Xs, 16, "logei", best_f=float(y.max()))
    out["topk_k16"] = bits(val) + bits(idx) + list(eng.sweep_stats())
    Y = np.stack([y, np.sin(3 * X).sum(1)], 1)
    sts = eng.fit_outputs(t(X), t(Y), [kp, kp.replace(outputscale=1.5)])
    bv, bi = eng.acquire_multi(sts, Xs, "ucb", weights=[0.5, 1.0])
    out["multi_T2"] = bits(bv) + bits(bi)
    torch.cuda.synchronize()
    print(json.dumps(out))


def sequence(path):
    """The library's launches in a rocprofv3 kernel trace, in dispatch order, as "kernel grid workgroup" lines (kernel:
    the name with its template arguments, without the parameter list); a file of such lines is returned as it is."""
    if not path.endswith(".csv"):
        return open(path).read().splitlines()
    rows = [r for r in csv.DictReader(open(path)) if "gpx::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, what: "x".join(r[f"{what}_Size_{a}"] for a in "XYZ")
    name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "")
    return [f'{name(r)} grid {dims(r, "Grid")} workgroup {dims(r, "Workgroup")}' for r in rows]


def diff(old, new):
    a, b = sequence(old), sequence(new)
    delta = list(difflib.unified_diff(a, b, old, new, lineterm="", n=2))
    print("\n".join(delta))
    print(f"{len(a)} launches in old, {len(b)} in new: {'identical' if a == b else 'DIFFERENT'}")
    return 0 if a == b and a else 1


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "seq":
        print("\n".join(sequence(sys.argv[2])))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
