#!/usr/bin/env python3
"""Records the sweep's reported workspace sizes of one libgpx.so over the grid of tests/test_sweep_workspace_sizes.py.

    tools/sweep_workspace_sizes.py --lib PATH/libgpx.so --commit SHA > tests/golden/sweep_workspace_sizes.json

Run against the library of the commit whose sizes are to be pinned (the size functions need no GPU).  Each entry is
[arguments..., bytes]; bytes = -1 where the library rejects the arguments.
"""
import argparse
import ctypes
import json
import sys

N = [1, 128, 200, 256, 257, 300, 384, 640, 1000, 4096, 16384, 100096]
NRHS = [1, 3, 8]
M = [1, 255, 256, 257, 5000, 349440, 349441, 2**20, 2**20 + 1, 2**22]
K = [1, 16, 1024]


def sizes(lib):
    """{function name: [[args..., bytes], ...]} of the three size functions over the grid."""
    for f, nargs in (("gpx_sweep_workspace_size", 3), ("gpx_acquire_topk_workspace_size", 3),
                     ("gpx_sweep_multi_workspace_size", 2)):
        getattr(lib, f).argtypes = [ctypes.c_int64] * nargs + [ctypes.POINTER(ctypes.c_size_t)]
        getattr(lib, f).restype = ctypes.c_int

    def call(f, *args):
        b = ctypes.c_size_t()
        return b.value if getattr(lib, f)(*args, ctypes.byref(b)) == 0 else -1

    return {
        "gpx_sweep_workspace_size": [[n, r, m, call("gpx_sweep_workspace_size", n, r, m)]
                                     for n in N for r in NRHS for m in M],
        "gpx_acquire_topk_workspace_size": [[n, m, k, call("gpx_acquire_topk_workspace_size", n, m, k)]
                                            for n in N for m in M for k in K if k <= m],
        "gpx_sweep_multi_workspace_size": [[n, m, call("gpx_sweep_multi_workspace_size", n, m)] for n in N for m in M],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    a = ap.parse_args()
    out = {"commit": a.commit}
    out.update(sizes(ctypes.CDLL(a.lib)))
    json.dump(out, sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
