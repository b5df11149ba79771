#!/usr/bin/env python3
"""The launch sequence of the acquisition sweep's paths, for comparing two builds of libgpx.so.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/sweep_launch_trace.py run
    python3 tools/sweep_launch_trace.py seq OUT/..._kernel_trace.csv [--fold-finalize] > NEW.txt
    python3 tools/sweep_launch_trace.py diff OLD.txt NEW.txt [--fold-finalize]

`run` makes one call per path at n = 384 (three row tiles), m = 3000: the lazy pruned sweep (RBF d = 8, with the mean
bound; Matern d = 3, without), the chunked pruned sweep (d = 20), the top-k form (k = 16), the multi-output sweep
(T = 2), and the fused sweep at n = 200; then one call per remaining pass of the finalize family at the smallest shape
that reaches it: the posterior (two outputs), the sweep with scores_out (every acquisition, RBF and
scale_linear_matern52), the seeded span (m = 400 000 under both sweep orders), the multi-output top-k form (T = 2,
k = 16) and the SVGP predictive and acquisition (T = 2, M = 200); it prints each result's bits.  Run it under a kernel
trace (no counters) once per library (GPX_LIB selects one other than the tree's).  `seq` prints the (kernel name, grid,
workgroup) sequence of the library's kernels in such a trace, one launch per line; `diff` compares two of them (either
form); exit status 0: identical.  --fold-finalize replaces the name of every kernel of the finalize family
(FINALIZE_FAMILY) by one token, for two builds that split the family's passes differently: grid and workgroup of every
line are still compared.
"""
import csv
import difflib
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trace_names import kernel_name  # noqa: E402


def run():
    import numpy as np
    import torch

    from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale
    from oracle import gp_oracle as O

    dev = torch.device("cuda", 0)
    eng = GPEngine(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)
    bits = lambda x: [int(v) for v in x.reshape(-1).view(torch.int64).tolist()]
    # (an array's bits as one number: sha256 of its bytes, the leading 16 hex digits)
    digest = lambda x: hashlib.sha256(x.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
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
    # the remaining passes of the finalize family
    val, idx = eng.acquire_topk_multi(sts, Xs, 16, "logei", best_f=float(y.max()), weights=[0.5, 1.0])
    out["topk_multi_T2_k16"] = bits(val) + bits(idx) + list(eng.sweep_stats())
    st2 = eng.fit(t(X), t(Y), kp)
    mean, var = eng.posterior(st2, Xs, y_mean=[0.1, -0.2], y_scale=[1.5, 0.5])
    out["posterior_nrhs2"] = [digest(mean), digest(var)]
    for kind in ("rbf", "scale_linear_matern52"):
        X, y, kp, Xs = problem(384, 8, kind)
        st = eng.fit(t(X), t(y), kp)
        for acq in ("logei", "ei", "ucb", "variance"):
            bv, bi, sc = eng.acquire(st, Xs, acq, best_f=float(y.max()), beta=4.0, return_scores=True)
            out[f"scores_{kind}_{acq}"] = bits(bv) + bits(bi) + [digest(sc)]
    X, y = O.synthetic_problem(384, 4, 21)
    st = eng.fit(t(X), t(y), KernelParams("rbf", botorch_default_lengthscale(4), linear_variance=0.3, noise=1e-4))
    Xl = t(O.sobol_candidates(400_000, 4, 22))
    for order in (0, 1):
        eng.set_option("sweep_order", order)
        bv, bi = eng.acquire(st, Xl, "logei", best_f=float(y.max()))
        out[f"seeded_order{order}"] = bits(bv) + bits(bi) + list(eng.sweep_stats())
    rng = np.random.default_rng(5)
    T, M, d = 2, 200, 4
    vchol = np.tril(0.3 * rng.standard_normal((T, M, M)) / np.sqrt(M), -1) + 0.5 * np.eye(M)
    params = [KernelParams("scale_linear_matern52", list(0.8 + rng.random(d)), outputscale=0.5 + 0.1 * i,
                           noise=1e-3 * (1 + i), const_mean=0.1 * i - 0.2,
                           linear_variance=list(0.05 + 0.1 * rng.random(d))) for i in range(T)]
    prep = eng.svgp_prepare(params, t(rng.standard_normal((T, M, d))), t(rng.standard_normal((T, M))), t(vchol))
    Xv = t(rng.standard_normal((m, d)))
    out["svgp_predict"] = [digest(x) for x in eng.svgp_predict(prep, Xv)]
    val, idx, sc = eng.svgp_acquire(prep, Xv, 16, "logei", best_f=0.5, weights=[0.5, 0.5], y_mean=[0.1, -0.2],
                                    y_scale=[1.5, 0.5], return_scores=True)
    out["svgp_acquire_T2"] = bits(val) + bits(idx) + [digest(sc)]
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
    name = lambda r: kernel_name(r["Kernel_Name"])
    return [f'{name(r)} grid {dims(r, "Grid")} workgroup {dims(r, "Workgroup")}' for r in rows]


FINALIZE_FAMILY = ("finalize_kernel", "multi_bound_select_kernel", "seed_select_kernel", "seed_prune_kernel",
                   "argmax_final_kernel", "svgp_finalize_kernel", "svgp_objective_kernel")
_FAMILY = re.compile(r"^gpx::(%s)\b\S*" % "|".join(FINALIZE_FAMILY))


def fold(lines):
    return [_FAMILY.sub("gpx::<finalize family>", ln) for ln in lines]


def diff(old, new, folded=False):
    a, b = sequence(old), sequence(new)
    if folded:
        a, b = fold(a), fold(b)
    delta = list(difflib.unified_diff(a, b, old, new, lineterm="", n=2))
    print("\n".join(delta))
    print(f"{len(a)} launches in old, {len(b)} in new: {'identical' if a == b else 'DIFFERENT'}")
    return 0 if a == b and a else 1


if __name__ == "__main__":
    folded = "--fold-finalize" in sys.argv
    argv = [a for a in sys.argv if a != "--fold-finalize"]
    if len(argv) == 2 and argv[1] == "run":
        run()
    elif len(argv) == 3 and argv[1] == "seq":
        lines = sequence(argv[2])
        print("\n".join(fold(lines) if folded else lines))
    elif len(argv) == 4 and argv[1] == "diff":
        sys.exit(diff(argv[2], argv[3], folded))
    else:
        sys.exit(__doc__)
