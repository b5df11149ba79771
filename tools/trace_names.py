"""Kernel names of a rocprofv3 --kernel-trace CSV, for the tools that read one."""


def kernel_name(full):
    """A traced kernel's name without `void ` and its parameter list: the text before the last balanced (...) group.
    Template arguments may hold parentheses of their own, as in finalize_kernel<(gpx::FinalizePass)2>."""
    full = full.replace("void ", "").rstrip()
    depth = 0
    for i in range(len(full) - 1, -1, -1):
        depth += (full[i] == ")") - (full[i] == "(")
        if depth == 0:
            return full[:i] if full[i] == "(" else full
    return full
