#!/usr/bin/env python3
"""Where the device idles in the last bench.py step of a rocprofv3 --kernel-trace CSV: the cost of the
pruned sweep's tail read-back that the device sees.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o bench -- python3 bench.py --gpus 1 --steps 7 --warmup 1
    python3 tools/tail_wait_gap.py OUT/bench_kernel_trace.csv LABEL

The last traced step is the library's launches from the last Gram launch on.  One JSON line: the step's launches, span
and busy time, the gap in front of argmax_final_kernel (the end of the tail's last launch to its start: with the
read-back the host enqueues it only after the wait) and the step's five longest gaps with the kernels on either side.
"""
import csv
import json
import sys

from trace_names import kernel_name


def main():
    path, label = sys.argv[1], sys.argv[2]
    rows = [r for r in csv.DictReader(open(path)) if "gpx::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    start = [i for i, r in enumerate(rows) if "gram" in r["Kernel_Name"]][-1]
    step = rows[start:]
    name = lambda r: kernel_name(r["Kernel_Name"]).replace("gpx::", "")  # noqa: E731
    t0 = int(step[0]["Start_Timestamp"])
    end, gaps, argmax_gap = int(step[0]["End_Timestamp"]), [], None
    for prev, r in zip(step, step[1:]):
        gap = (int(r["Start_Timestamp"]) - end) / 1e3
        gaps.append((round(gap, 2), name(prev)[:60], name(r)[:60], round((int(r["Start_Timestamp"]) - t0) / 1e3, 1)))
        if name(r).startswith("argmax_final_kernel"):
            argmax_gap = round(gap, 2)
        end = max(end, int(r["End_Timestamp"]))
    busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in step) / 1e3
    print(json.dumps({"file": label, "launches": len(step), "span_us": round((end - t0) / 1e3, 1),
                      "busy_us": round(busy, 1), "gap_before_argmax_us": argmax_gap,
                      "gaps_over_0_us": round(sum(g[0] for g in gaps if g[0] > 0), 1),
                      "longest_gaps": sorted(gaps, reverse=True)[:5]}))


if __name__ == "__main__":
    main()
