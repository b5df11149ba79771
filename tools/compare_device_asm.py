#!/usr/bin/env python3
"""Compares the device assembly of two builds of one translation unit, function by function.

    tools/compare_device_asm.py OLD.s NEW.s

The files are the build's lib/obj/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s.  A host-only change must leave every device
function as it was, but may move functions in the file (the emission order follows the order in which host code first
instantiates each template), which renumbers the local labels.  So each function's text (its instructions, kernel
descriptor and resource symbols) is compared after dropping `;` comments and the function index inside local labels
(.LBB86_24 and .LBB98_24 count as the same label).  Exit status 0: same symbols, same text.

    tools/compare_device_asm.py --opcodes OLD.s NEW.s

also prints, for every function that differs, its opcode histogram in both builds as "opcode old new": the arithmetic
that carries a kernel's cost and rounding (MFMA, v_exp, v_fma / v_fmac, fp64 add / mul, conversions) always, any other
opcode where the counts differ (`*`).  A change that only reorders a kernel's instructions leaves every count as it was.
(NEW.s may be several units' files concatenated, for a unit that was split.)
"""
import collections
import re
import sys

_FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
_LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")
_WATCHED = re.compile(r"v_mfma|v_exp|v_fma|v_add_f64|v_mul_f64|v_cvt")


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


def opcodes(lines):
    """Histogram of a function's instructions (labels and directives left out)."""
    return collections.Counter(ln.split()[0] for ln in lines if not ln.startswith(".") and not ln.endswith(":"))


def main():
    args = [a for a in sys.argv[1:] if a != "--opcodes"]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = functions(args[0]), functions(args[1])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(f for f in set(old) & set(new) if old[f] != new[f])
    for tag, names in (("only in old", gone), ("only in new", added), ("differs", differ)):
        for f in names:
            print(f"{tag}: {f}")
    if "--opcodes" in sys.argv:
        for f in differ:
            a, b = opcodes(old[f]), opcodes(new[f])
            print(f"opcodes of {f}: {sum(a.values())} instructions in old, {sum(b.values())} in new")
            for op in sorted(set(a) | set(b)):
                if a[op] != b[op] or _WATCHED.match(op):
                    print(f"  {op} {a[op]} {b[op]}{' *' if a[op] != b[op] else ''}")
    lines = sum(len(v) for v in new.values())
    print(f"{len(old)} functions in old, {len(new)} in new ({lines} lines compared): "
          f"{len(gone)} removed, {len(added)} added, {len(differ)} differ")
    sys.exit(1 if gone or added or differ else 0)


if __name__ == "__main__":
    main()
