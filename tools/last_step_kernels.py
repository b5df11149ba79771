"""Per-kernel launches and time of the last bench.py step in a rocprofv3 --kernel-trace CSV.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o bench -- python3 bench.py --gpus 1 --steps 7 --warmup 1
    python3 tools/last_step_kernels.py OUT/bench_kernel_trace.csv LABEL

The last traced step is the library's launches from the last Gram launch on.  One JSON line: per kernel its launches and
their time, and apart the launches under 8 us (the empty tail rounds' and other tiny ones).
"""
import csv, json, sys, collections
from trace_names import kernel_name
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
names = [r["Kernel_Name"] for r in rows]
start = [i for i, n in enumerate(names) if "gram" in n and "gpx::" in n][-1]
agg = collections.OrderedDict()
t0 = int(rows[start]["Start_Timestamp"]); t1 = t0
for r in rows[start:]:
    nm = r["Kernel_Name"]
    if "gpx::" not in nm:
        continue
    nm = kernel_name(nm)
    d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    a = agg.setdefault(nm, [0, 0.0, 0, 0.0])
    a[0] += 1; a[1] += d
    if d < 8.0: a[2] += 1; a[3] += d   # launches under 8 us (empty or tiny)
    t1 = max(t1, int(r["End_Timestamp"]))
print(json.dumps({"file": sys.argv[2], "span_us": (t1 - t0) / 1e3, "busy_us": sum(a[1] for a in agg.values()),
                  "kernels": {k: {"launches": v[0], "us": round(v[1], 1), "under_8us": v[2], "their_us": round(v[3], 1)}
                              for k, v in agg.items()}}))
