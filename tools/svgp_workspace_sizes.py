#!/usr/bin/env python3
"""Records the SVGP calls' reported workspace sizes of one libgpx.so over the grid of tests/test_svgp_workspace_sizes.py.

    tools/svgp_workspace_sizes.py --lib PATH/libgpx.so --commit SHA > tests/golden/svgp_workspace_sizes.json

Run against the library of the commit whose sizes are to be pinned (the size functions need no GPU).  Each entry is
[arguments..., bytes]; bytes = -1 where the library rejects the arguments.
"""
import argparse
import ctypes
import json
import sys

M = [1, 64, 128, 129, 130, 200, 2048, 65536, 65537]
NTASK = [1, 3, 8, 64, 65]
N = [1, 127, 128, 129, 700, 100000]
CHUNK = [0, 1, 128, 129, 300, 16384, 2**20, 2**20 + 1, -1]
MCAND = [1, 255, 256, 257, 5000, 2**20 + 1]
FUNCTIONS = {  # name: the grids of its arguments, in order
    "gpx_svgp_prepare_workspace_size": (M, NTASK),
    "gpx_svgp_predict_workspace_size": (M, MCAND),
    "gpx_svgp_fit_collapsed_workspace_size": (M, N, NTASK, CHUNK),
    "gpx_svgp_bound_grad_workspace_size": (M, N, NTASK, CHUNK),
}


def grid(axes):
    out = [[]]
    for axis in axes:
        out = [row + [v] for row in out for v in axis]
    return out


def sizes(lib):
    """{function name: [[args..., bytes], ...]} of the four size functions over the grid."""
    res = {}
    for name, axes in FUNCTIONS.items():
        f = getattr(lib, name)
        f.argtypes = [ctypes.c_int64] * len(axes) + [ctypes.POINTER(ctypes.c_size_t)]
        f.restype = ctypes.c_int
        rows = []
        for args in grid(axes):
            b = ctypes.c_size_t()
            rows.append(args + [b.value if f(*args, ctypes.byref(b)) == 0 else -1])
        res[name] = rows
    return res


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
