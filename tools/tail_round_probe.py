"""The columns the live tail rounds of the lazy pruned sweep handle, read from the stage descriptors and
survivor counts a call leaves in its workspace (gpx_sweep_layout.h: SR_DESC, SR_COUNT behind the main part).

A call over one chunk's candidates has one tail round (and the leading block as its seed), so it leaves that round's
descriptors (slot 1: the gather's set, then one per compaction: buf, col0, ncols, ntiles, list) and the survivors after
every stage (count[0]: the head's).  After the whole call (one span of 2^20, seeded from the head's bound) the later
rounds have overwritten them, but count[0] is still the survivors of the last span's prune pass, the seed's columns
left out, and sweep_stats[1] - 1024 is what the tail computed to the end.  In the mean-first order (sweep_order 1, the
default for this call) descriptor slot 0 of the whole call is no longer the span's contiguous column set: the list-driven
head overwrites it with the set S1 its first prune pass kept (buf 0, col0 0, ncols = |S1|, ntiles = the head's groups,
list 2), and count[9] is |S1| again ("s1"; count[8] is the seed list's length).  One JSON line per case.  The library is
the tree's, or GPX_LIB's.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", default="0,1000")
a = ap.parse_args()
D, M, N = 8, 1 << 20, 4096
dev = torch.device("cuda", 0)
eng = GPEngine(0)
kp = KernelParams("rbf", botorch_default_lengthscale(D), noise=1e-4)


def workspace_state(npad, m):
    ws = eng._ws["sweep"]
    cap = ((1 << 30) // 8 // npad) // 256 * 256
    C = min((m + 255) // 256 * 256, cap)
    nrec = (m + 255) // 256 + 1
    main = npad * C * 8 + (npad // 64) * C * 8 + (npad // 128) * C * 8 + 2 * nrec * 8
    at = (-ws.data_ptr()) % 256 + (main + 255) // 256 * 256
    torch.cuda.synchronize()
    return (ws[at:at + 256].view(torch.int32).reshape(8, 8)[:, :5].tolist(),
            ws[at + 256:at + 296].view(torch.int32).tolist())


for seed in (int(s) for s in a.seeds.split(",")):
    X, y = synthetic.problem(N, D, seed)
    st = eng.fit(torch.tensor(X, device=dev), torch.tensor(y, device=dev), kp)
    Xs = torch.tensor(synthetic.sobol(M, D, seed + 1), device=dev)
    npad = st.npad
    C = ((1 << 30) // 8 // npad) // 256 * 256
    for name, m in (("first_chunk", C), ("whole_call", M)):
        bv, bi = eng.acquire(st, Xs[:m], "logei", best_f=float(y.max()))
        stats = eng.sweep_stats()
        desc, count = workspace_state(npad, m)
        print(json.dumps({"case": f"seed{seed}_{name}", "m": m, "sweep_stats": list(stats), "best": int(bi.item()),
                          "descriptors": desc[:7], "counts": count[:7], "seed": count[8], "s1": count[9]}),
              flush=True)
