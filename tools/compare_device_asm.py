#!/usr/bin/env python3
"""Compares the device assembly of two builds of one translation unit, function by function.

    tools/compare_device_asm.py OLD.s NEW.s

The files are the build's lib/obj/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s.  A host-only change must leave every device
function as it was, but may move functions in the file (the emission order follows the order in which host code first
instantiates each template), which renumbers the local labels.  So each function's text (its instructions, kernel
descriptor and resource symbols) is compared after dropping `;` comments and the function index inside local labels
(.LBB86_24 and .LBB98_24 count as the same label).  Exit status 0: same symbols, same text.
"""
import re
import sys

_FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
_LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")


def functions(path):
    """{symbol: normalised lines} of every function in the file."""
    out, name = {}, None
    for line in open(path):
        m = _FUNC.match(line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None:
            continue
        if line.lstrip().startswith((".section\t.AMDGPU.csdata", ".amdgpu_metadata")):
            name = None  # the per-function comment block / the file's metadata: not code
            continue
        line = _LABEL.sub(lambda g: "." + g.group(1), line.split(";", 1)[0]).strip()
        if line:
            out[name].append(line)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(f for f in set(old) & set(new) if old[f] != new[f])
    for tag, names in (("only in old", gone), ("only in new", added), ("differs", differ)):
        for f in names:
            print(f"{tag}: {f}")
    lines = sum(len(v) for v in new.values())
    print(f"{len(old)} functions in old, {len(new)} in new ({lines} lines compared): "
          f"{len(gone)} removed, {len(added)} added, {len(differ)} differ")
    sys.exit(1 if gone or added or differ else 0)


if __name__ == "__main__":
    main()
