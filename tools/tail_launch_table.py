#!/usr/bin/env python3
"""The launches of the lazy pruned sweep's tail in a rocprofv3 --kernel-trace CSV of bench.py.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o bench -- python3 bench.py --gpus 1 --steps 7 --warmup 1
    python3 tools/tail_launch_table.py OUT/bench_kernel_trace.csv [--launches]

The last traced step is the library's launches from the last Gram launch on.  A tail round starts at a KSTAR_GATHER
launch (kstar_mfma_kernel<.., 2>) and ends before the next launch that is none of the tail's kernels.  The host
enqueues a super-chunk's first round with the doubling stages (more than three stage launches) and the later rounds
with at most three; on a problem whose survivors per super-chunk fit one round (the bench problem: sweep_stats shows
1,173 survivors in all against rounds of 32,768) exactly the first rounds are live.  Prints, per family, launches and
time of the live and of the empty rounds; every live gather and compaction launch; with --launches every tail launch
(kernel, grid in workgroups, start relative to the step, duration).
"""
import csv
import sys
from collections import defaultdict

from trace_names import kernel_name

TAIL = ("kstar_mfma_kernel", "trmm_stage_dual_kernel", "finalize_kernel", "prune_compact_kernel", "topk_pool_kernel")


def short(name):
    return kernel_name(name).replace("gpx::", "")


def main():
    path = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    rows = [r for r in csv.DictReader(open(path)) if "gpx::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    start = [i for i, r in enumerate(rows) if "gram" in r["Kernel_Name"]][-1]
    step = rows[start:]
    t0 = int(step[0]["Start_Timestamp"])
    rounds, cur = [], None
    for r in step:
        nm = short(r["Kernel_Name"])
        gather = nm.startswith("kstar_mfma_kernel") and nm.rstrip(">").endswith(", 2")
        if gather:
            cur = []
            rounds.append(cur)
        elif cur is not None and not nm.startswith(TAIL[1:]):
            cur = None
        if cur is not None:
            wgs = 1
            for a in "XYZ":
                wgs *= int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"])
            cur.append((nm, wgs, (int(r["Start_Timestamp"]) - t0) / 1e3,
                        (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    fam = defaultdict(lambda: [0, 0.0, 0, 0.0])  # live launches, live us, empty launches, empty us
    for i, rd in enumerate(rounds):
        live = sum(1 for l in rd if l[0].startswith("trmm_stage_dual_kernel")) > 3
        for nm, wgs, at, dur in rd:
            f = fam[nm]
            f[0 if live else 2] += 1
            f[1 if live else 3] += dur
            if "--launches" in sys.argv:
                print(f"round {i:2d} {'live ' if live else 'empty'} {nm[:44]:44s} wgs={wgs:6d} at={at:9.1f}us dur={dur:7.2f}us")
            elif live and (nm.startswith("kstar") or nm.startswith("prune_compact")):
                print(f"round {i:2d} live  {nm[:44]:44s} wgs={wgs:6d} at={at:9.1f}us dur={dur:7.2f}us")
    print(f"{len(rounds)} rounds, {sum(len(r) for r in rounds)} launches")
    print(f"{'family':46s} {'live':>14s} {'empty':>14s}")
    tot = [0, 0.0, 0, 0.0]
    for nm, f in sorted(fam.items()):
        print(f"{nm[:46]:46s} {f[0]:4d} {f[1]:8.1f}us {f[2]:4d} {f[3]:8.1f}us")
        tot = [a + b for a, b in zip(tot, f)]
    print(f"{'all':46s} {tot[0]:4d} {tot[1]:8.1f}us {tot[2]:4d} {tot[3]:8.1f}us")
    print(f"step span {(int(step[-1]['End_Timestamp']) - t0) / 1e3:.1f}us over {len(step)} launches")


if __name__ == "__main__":
    main()
