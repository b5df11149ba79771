"""Which form of the head mean bound (csrc/gpx_mubound.hip) each workgroup of 256 candidates takes
(gpx_debug_mu_bound_f64's two counters, written by mu_classify): one
JSON line per problem with the workgroups on mu_bound_kernel, on the fp64 factorised form and on the fp32 one, and the
largest Y_c of the candidates.  Problems: the bench step (n = 4096, d = 8, seed 0, 2^20 Sobol candidates), the seed-1000
problem and n = 1024."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, synthetic, _capi

D, M = 8, 1 << 20
dev = torch.device("cuda", 0)
eng = GPEngine(0)
lib = eng.lib
ls = botorch_default_lengthscale(D)
kp = KernelParams("rbf", ls, noise=1e-4)
for n, seed, cseed in ((4096, 0, 1), (4096, 1000, 1001), (1024, 0, 1)):
    X, y = synthetic.problem(n, D, seed)
    Xs = synthetic.sobol(M, D, cseed)
    Xd, Xsd = torch.tensor(X, device=dev), torch.tensor(Xs, device=dev)
    st = eng.fit(Xd, torch.tensor(y, device=dev), kp)
    alpha = st.alpha[:, 0].contiguous()
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_mu_bound_workspace_size(n, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    ma = torch.empty(M, dtype=torch.float64, device=dev)
    sl = torch.empty(M, dtype=torch.float64, device=dev)
    pc = kp.to_c(D)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    _capi.check(lib.gpx_debug_mu_bound_f64(eng.handle, ctypes.byref(pc), n, p(Xd), Xd.stride(0), p(alpha), p(Xsd), M,
                                           Xsd.stride(0), p(ma), p(sl), p(ws), ws.numel()), eng.handle)
    torch.cuda.synchronize()
    off = (-ws.data_ptr()) % 256
    fallback = int(ws[off:off + 8].view(torch.int64).item())
    fp64form = int(ws[off + 160:off + 168].view(torch.int64).item())
    s = X / ls
    c = s.mean(axis=0)
    m2 = float(((s - c) ** 2).sum(axis=1).max())
    yc = 1.4426950408889634 * np.sqrt(m2 * ((Xs / ls - c) ** 2).sum(axis=1))
    wg = yc.reshape(-1, 256).max(axis=1)
    print(json.dumps({"n": n, "seed": seed, "workgroups": M // 256, "mu_bound_kernel": fallback, "fp64_form": fp64form,
                      "fp32_form": M // 256 - fallback - fp64form, "M2": m2, "max_Yc": float(yc.max()),
                      "median_workgroup_max_Yc": float(np.median(wg)),
                      "median_slack_over_abs_mu": float((sl / ma.abs().clamp_min(1e-300)).median())}), flush=True)
