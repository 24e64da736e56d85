"""CPU: bench.py's --full switch and --dump-outputs writer.

A plain run keeps only the timed steps (the extras' opt-out flags are all on); --full turns them on again and
the opt-out flags still subtract from it.  dump_outputs writes float32 / float64 .npy files, whole when small
and as the same fixed sample on every call when above DUMP_MAX_ELEMS."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return _bench().parse()


def test_plain_run_has_no_extras(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None
    assert a.no_kernel_timing and a.no_cpu_baseline and a.no_cpu_legs
    assert (a.steps, a.warmup, a.workload, a.dtype) == (5, 2, "sample", "fp32")


def test_full_run_keeps_the_opt_outs(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert a.full and not (a.no_kernel_timing or a.no_cpu_baseline or a.no_cpu_legs)
    a = _parse(monkeypatch, ["--full", "--no-cpu-baseline", "--dump-outputs", "d"])
    assert a.no_cpu_baseline and not a.no_kernel_timing and a.dump_outputs == "d"


def test_dump_outputs_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    arrays = {"small": torch.arange(6, dtype=torch.bfloat16).reshape(2, 3), "wide": torch.ones(3, dtype=torch.float64),
              "big": big, "losses": [0.5, 1.5]}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert got["small"].dtype == np.float32 and got["small"].shape == (2, 3)
    assert np.array_equal(got["small"], np.arange(6, dtype=np.float32).reshape(2, 3))
    assert got["wide"].dtype == np.float64 and got["losses"].dtype == np.float64
    assert np.array_equal(got["losses"], [0.5, 1.5])
    # the sample: DUMP_MAX_ELEMS elements of the flat array at sorted positions, identical call to call
    s = got["big"]
    assert s.dtype == np.float32 and s.shape == (1000,)
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 5000 and len(np.unique(s)) > 800
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in arrays)
