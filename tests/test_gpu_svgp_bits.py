"""The four SVGP calls keep their bits (gpx_svgp_fit_collapsed_f64, gpx_svgp_bound_grad_f64, gpx_svgp_prepare_f64,
gpx_svgp_predict_f64) against tests/golden/svgp_bits.json, recorded from the commit before their workspaces got one
layout (csrc/gpx_svgp_layout.h) and their drivers shared steps.

Cases, on the problems of tests/sgpr_ref.py: shape 3 (n 400, M 130, d 5, T 2: Mpad = 256, two row tiles, padded rows) at
the default chunk; shape 2 (n 700, M 200, T 3) at chunk = 128 and at the default; shape 4 (M 64, T 8: one tile, the widest
task batch of the shapes).  Per case the fixture holds the sha256 of the host-made inputs (checked first: a mismatch
there is the host's, not the kernels') and of every output: the fit's vmean, vchol, bound, info; the gradient's out,
info; prepare's (from the fit's result) W, W2, alpha, info; predict's mean, var, score at 256 seeded candidates.  Outputs
are allocated zeroed, so an element a call leaves alone cannot change a digest.

One more case pins the choice of the chunk width from ws_bytes end to end, through the raw C entry points on shape 2.
The chunk-width regions are ldk = chunk rounded up to 256 columns wide, so the sizes of chunk = 128 and chunk = 256 are
the same number, and a call given the chunk = 128 size runs 256 wide.  Hence a workspace of size(chunk = 256) - 256
bytes lies below every size and is refused (the recorded status), and the first workspace that makes the library choose
is size(chunk = 384) - 256 bytes of the call's own size function: it must run 256 wide again, with the digests of the
chunk = 128 case.  To record the fixture again (GPX_LIB selects the library):

    python tests/test_gpu_svgp_bits.py OUT.json
"""
import ctypes
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from bayesianoptimizer_amd.engine import KernelParamsC
from tests import sgpr_ref as R

pytestmark = pytest.mark.gpu
CASES = {"shape 3 default chunk": (3, 0), "shape 2 chunk 128": (2, 128), "shape 2 default chunk": (2, 0),
         "shape 4 default chunk": (4, 0)}
CHOOSER = "shape 2 workspace below the chunk 384 size"
NCAND = 256
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svgp_bits.json")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def shas(**tensors):
    return {k: sha(v.cpu().numpy()) for k, v in tensors.items()}


def ptr(a):
    return ctypes.c_void_p(a.data_ptr())


class Problem:
    """A shape's problem on the device, its kernel parameters as the C ABI takes them, and the candidates."""

    def __init__(self, engine, shape):
        pb = R.problem(shape)
        self.T, self.M, self.d = pb.Z.shape
        self.n = pb.X.shape[0]
        self.kps = pb.kps
        self.pcs = (KernelParamsC * self.T)(*[p.to_c(self.d) for p in pb.kps])
        Xq = R.SHAPES[shape][4] * np.random.default_rng(500 + shape).standard_normal((NCAND, self.d))
        self.inputs_sha256 = sha(pb.X, pb.Y, pb.Z, Xq, bytes(self.pcs))
        self.engine = engine
        self.X, self.Y, self.Z, self.Xq = (torch.tensor(a, device=engine.device) for a in (pb.X, pb.Y, pb.Z, Xq))

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=self.engine.device)

    def workspace(self, size_fn, *args):
        nb = ctypes.c_size_t()
        assert getattr(self.engine.lib, size_fn)(*args, ctypes.byref(nb)) == _capi.GPX_OK
        return torch.empty(nb.value, dtype=torch.uint8, device=self.engine.device), nb.value

    def fit(self, chunk, ws_bytes=None):
        """(status, vmean, vchol, bound, info) of the C call; ws_bytes: told instead of the workspace's own size."""
        e, T, M, d = self.engine, self.T, self.M, self.d
        vmean, vchol, bound = self.zeros(T, M), self.zeros(T, M, M), self.zeros(T, _capi.SVGP_BOUND_NOUT)
        info = self.zeros(T, dtype=torch.int32)
        ws, nb = self.workspace("gpx_svgp_fit_collapsed_workspace_size", M, self.n, T, chunk)
        e._bind_stream()
        st = e.lib.gpx_svgp_fit_collapsed_f64(e.handle, self.pcs, T, M, R.JITTER, ptr(self.Z), d, M * d, ptr(self.X),
                                              self.n, d, ptr(self.Y), T, ptr(vmean), M, ptr(vchol), M, M * M,
                                              ptr(bound), ptr(info), ptr(ws), nb if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return st, vmean, vchol, bound, info

    def grad(self, chunk, ws_bytes=None):
        e, T, M, d = self.engine, self.T, self.M, self.d
        out, info = self.zeros(T, _capi.SVGP_GRAD_NOUT), self.zeros(T, dtype=torch.int32)
        ws, nb = self.workspace("gpx_svgp_bound_grad_workspace_size", M, self.n, T, chunk)
        e._bind_stream()
        st = e.lib.gpx_svgp_bound_grad_f64(e.handle, self.pcs, T, M, R.JITTER, ptr(self.Z), d, M * d, ptr(self.X),
                                           self.n, d, ptr(self.Y), T, ptr(out), ptr(info), ptr(ws),
                                           nb if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return st, out, info

    def prepare(self, vmean, vchol):
        e, T, M, d = self.engine, self.T, self.M, self.d
        Mpad = e.padded_n(M)
        W, W2, alpha = self.zeros(T, Mpad, Mpad), self.zeros(T, Mpad, Mpad), self.zeros(T, Mpad)
        info = self.zeros(T, dtype=torch.int32)
        ws, nb = self.workspace("gpx_svgp_prepare_workspace_size", M, T)
        e._bind_stream()
        st = e.lib.gpx_svgp_prepare_f64(e.handle, self.pcs, T, M, R.JITTER, ptr(self.Z), d, M * d, ptr(vmean), M,
                                        ptr(vchol), M, M * M, ptr(W), ptr(W2), ptr(alpha), ptr(info), ptr(ws), nb)
        torch.cuda.synchronize()
        return st, W, W2, alpha, info


def digest(engine, shape, chunk):
    pb = Problem(engine, shape)
    st, vmean, vchol, bound, finfo = pb.fit(chunk)
    assert st == _capi.GPX_OK and int(finfo.abs().sum()) == 0
    st, out, ginfo = pb.grad(chunk)
    assert st == _capi.GPX_OK and int(ginfo.abs().sum()) == 0
    st, W, W2, alpha, pinfo = pb.prepare(vmean, vchol)
    assert st == _capi.GPX_OK and int(pinfo.abs().sum()) == 0
    prep = {"Z": pb.Z, "W": W, "W2": W2, "alpha": alpha, "params": pb.kps, "M": pb.M}
    mean, var, score = engine.svgp_predict(prep, pb.Xq)
    return {"inputs_sha256": pb.inputs_sha256,
            "fit": shas(vmean=vmean, vchol=vchol, bound=bound, info=finfo),
            "grad": shas(out=out, info=ginfo),
            "prepare": shas(W=W, W2=W2, alpha=alpha, info=pinfo),
            "predict": shas(mean=mean, var=var, score=score)}


def chooser_digest(engine):
    """Shape 2 through the raw entry points, told a workspace 256 bytes short of a size: of chunk = 256 (refused: the
    statuses), and of chunk = 384 (the library chooses the width: the digests)."""
    pb = Problem(engine, 2)
    res = {"inputs_sha256": pb.inputs_sha256}
    for name, call, size_fn in (("fit", pb.fit, "gpx_svgp_fit_collapsed_workspace_size"),
                                ("grad", pb.grad, "gpx_svgp_bound_grad_workspace_size")):
        size = {c: pb.workspace(size_fn, pb.M, pb.n, pb.T, c)[1] for c in (128, 256, 384)}
        assert size[128] == size[256] < size[384]
        res[name + " status below the chunk 256 size"] = call(256, ws_bytes=size[256] - 256)[0]
        st, *outs, info = call(384, ws_bytes=size[384] - 256)
        assert st == _capi.GPX_OK and int(info.abs().sum()) == 0
        names = ("vmean", "vchol", "bound") if name == "fit" else ("out",)
        res[name] = shas(**dict(zip(names, outs)), info=info)
    return res


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_svgp_bits(engine, golden, case):
    want = golden[case]
    got = digest(engine, *CASES[case])
    assert got["inputs_sha256"] == want["inputs_sha256"], "the host-made inputs differ from the recorded ones"
    assert got == want


def test_chunk_width_chosen_from_the_workspace_size(engine, golden):
    want = golden[CHOOSER]
    got = chooser_digest(engine)
    assert got["inputs_sha256"] == want["inputs_sha256"], "the host-made inputs differ from the recorded ones"
    assert got == want
    assert got["fit status below the chunk 256 size"] == got["grad status below the chunk 256 size"] \
        == _capi.GPX_INVALID_ARG
    narrow = golden["shape 2 chunk 128"]
    assert got["fit"] == narrow["fit"] and got["grad"] == narrow["grad"]


if __name__ == "__main__":
    from bayesianoptimizer_amd import GPEngine

    eng = GPEngine(0)
    out = {case: digest(eng, *args) for case, args in CASES.items()}
    out[CHOOSER] = chooser_digest(eng)
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} cases -> {sys.argv[1]}")
