"""bench.py's --dump-outputs on the CPU: the float64 files are exact for 64-bit words, stay within their budget by a
seeded sample of rows, and are the same from run to run.  (Their content, the last timed step's histogram, is checked
against the oracle in tests/test_gpu_parity.py.)"""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("tatajuba_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_u64_columns_are_exact():
    b = _bench()
    w = np.array([0, 1, 0xFFFFFFFF, 1 << 32, (1 << 53) + 1, (1 << 64) - 1, 0x0123456789ABCDEF], dtype=np.uint64)
    lo, hi = b.u64_columns(w)
    assert lo.dtype == hi.dtype == np.float64
    assert (lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32)) == w).all()


def test_dump_outputs_within_budget_writes_every_row(tmp_path):
    b = _bench()
    rec = {"kept_records": np.arange(50.0).reshape(10, 5), "context_index": np.arange(6.0).reshape(3, 2)}
    b.dump_outputs(str(tmp_path / "d"), rec, {"summary": [10, 3, 7]})
    assert sorted(os.listdir(tmp_path / "d")) == ["context_index.npy", "kept_records.npy", "summary.npy"]
    for name, a in rec.items():
        got = np.load(tmp_path / "d" / (name + ".npy"))
        assert got.dtype == np.float64 and (got == a).all()
    assert np.load(tmp_path / "d" / "summary.npy").tolist() == [10.0, 3.0, 7.0]


def test_dump_outputs_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BYTES", 8 * 4000)
    rec = {"a": np.arange(6000.0).reshape(2000, 3), "b": np.arange(2000.0)}      # 64 000 bytes: half the rows of each
    for d in ("x", "y"):
        b.dump_outputs(str(tmp_path / d), rec, {"summary": [2000]})
    total = 0
    for name, a in rec.items():
        x, y = (np.load(tmp_path / d / (name + ".npy")) for d in ("x", "y"))
        assert (x == y).all() and len(x) == len(a) // 2
        assert np.isin(x, a).all() and (np.diff(x if x.ndim == 1 else x[:, 0]) > 0).all()      # rows of the array, in order
        total += x.nbytes
    assert total <= 8 * 4000
    assert np.load(tmp_path / "x" / "summary.npy").tolist() == [2000.0]


def test_bench_refuses_a_run_without_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
