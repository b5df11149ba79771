"""bench.py --dump-outputs / --full: what a plain run prints and writes.

CPU: the writer itself (dump_outputs) on host tensors with the fields of a GPState: names, dtype, the fixed sample
positions, the size bound.  GPU: a small plain run in this process, twice, writes identical arrays (same arguments ->
same inputs -> same outputs) and prints a line without the fields that --full adds.
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("updates_per_s", "fit_ms", "update_breakdown_ms", "updates_roofline", "gram_roofline", "cpu_baseline",
             "exchange", "other_configs")


def _state(n, npad, seed):
    g = torch.Generator().manual_seed(seed)
    L = torch.tril(torch.rand((npad, npad), dtype=torch.float64, generator=g)) + torch.eye(npad, dtype=torch.float64)
    W = torch.triu(torch.rand((npad, npad), dtype=torch.float64, generator=g))
    alpha = torch.rand((npad, 1), dtype=torch.float64, generator=g)
    return types.SimpleNamespace(L=L, W=W, alpha=alpha, n=n, W_ready=True)


def test_dump_outputs_writes_named_fp64_arrays(tmp_path):
    n, npad = 100, 128
    states = [_state(n, npad, 1), _state(n, npad, 2)]
    probs = [(None, None, None, 0.0, 6), (None, None, None, 0.0, 7)]
    bv, bi = torch.tensor([0.25], dtype=torch.float64), torch.tensor([12345], dtype=torch.int64)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), bv, bi, states, probs, write_best=True)
    names = sorted(os.listdir(out))
    assert names == sorted(["best_value.npy", "best_index.npy"] + [f"{k}_u{u}.npy" for u in (6, 7)
                                                                    for k in ("alpha", "chol_sample", "winv_sample")])
    arrays = {f: np.load(out / f) for f in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    assert arrays["best_value.npy"].tolist() == [0.25] and arrays["best_index.npy"].tolist() == [12345.0]
    for st, u in zip(states, (6, 7)):
        assert np.array_equal(arrays[f"alpha_u{u}.npy"], st.alpha[:n].numpy())
        # the samples lie inside the n x n problem, in L's lower and W's upper triangle: never the padding, never the
        # undefined half (the test factors have zeros there, and strictly positive entries where they are defined)
        assert np.all(arrays[f"chol_sample_u{u}.npy"] > 0) and np.all(arrays[f"winv_sample_u{u}.npy"] > 0)
        vals = set(arrays[f"chol_sample_u{u}.npy"].tolist())
        assert vals <= set(st.L[:n, :n].numpy().ravel().tolist())
    # the same positions on every call: a second dump of the same states is identical; rank != 0 writes no best_*
    out2 = tmp_path / "dump2"
    bench.dump_outputs(str(out2), bv, bi, states, probs, write_best=False)
    assert "best_value.npy" not in os.listdir(out2)
    for f in os.listdir(out2):
        assert np.array_equal(np.load(out2 / f), arrays[f])
    # a factor-only state (no L^-T built) has no winv sample
    states[0].W_ready = False
    out3 = tmp_path / "dump3"
    bench.dump_outputs(str(out3), bv, bi, states[:1], probs[:1], write_best=False)
    assert sorted(os.listdir(out3)) == ["alpha_u6.npy", "chol_sample_u6.npy"]


def test_dump_sample_stays_inside_the_size_bound():
    # per problem two samples of fp64 entries; alpha (n x nrhs) and best_* are a few tens of KiB per problem beside them
    assert bench.dump_sample_size(1) == 1 << 20
    for problems in (1, 4, 8, 32, 256):
        assert 1 <= 16 * bench.dump_sample_size(problems) * problems <= 48 * 1000 * 1000


def test_options_parse():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.steps == 3 and a.warmup == 1 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "somewhere", "--no-cpu-baseline"])
    assert a.full and a.dump_outputs == "somewhere" and a.no_cpu_baseline
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path, capsys):
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "512", "--d", "4", "--m", "8192"]
    lines = []
    for i in (1, 2):
        bench.main(argv + ["--dump-outputs", str(tmp_path / f"d{i}")])
        lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    for d in lines:
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["dtype"] == "f64" and d["higher_is_better"] is True
        assert d["value"] == pytest.approx(8192 * 1e3 / d["ms_per_step"])
        assert not any(k in d for k in FULL_ONLY)
    assert lines[0]["best"] == lines[1]["best"]
    names = sorted(os.listdir(tmp_path / "d1"))
    assert names == ["alpha_u0.npy", "best_index.npy", "best_value.npy", "chol_sample_u0.npy", "winv_sample_u0.npy"]
    for f in names:
        a, b = np.load(tmp_path / "d1" / f), np.load(tmp_path / "d2" / f)
        assert a.dtype == np.float64 and np.isfinite(a).all() and np.array_equal(a, b)
    assert np.load(tmp_path / "d1" / "best_index.npy")[0] == lines[0]["best"]["index"]
    assert np.load(tmp_path / "d1" / "best_value.npy")[0] == lines[0]["best"]["value"]
    assert np.load(tmp_path / "d1" / "alpha_u0.npy").shape == (512, 1)
