"""`bench.py --dump-outputs DIR`: the last timed step's outputs as DIR/<name>.npy in float32, the same rows from run to run, at most
64 MB in all.  CPU only: the `stub` workload, and bench.dump_outputs itself with a lowered cap."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_stub_dumps_its_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "stub", "--steps", "3", "--warmup", "1", "--dump-outputs",
                        str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    a = np.load(tmp_path / "out" / "embeddings.npy")
    assert a.dtype == np.float32 and a.shape == (4, 8) and not a.any()     # one rank: rank 0's rows


def test_dump_keeps_a_fixed_row_sample_under_the_cap(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * 1024)
    big = np.arange(1000 * 16, dtype=np.float64).reshape(1000, 16)          # 64 KB as float32
    small = np.ones((10, 16), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    s = np.load(tmp_path / "a" / "small.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert a.nbytes + s.nbytes <= 40 * 1024 and a.shape[1] == 16 and 0 < a.shape[0] < 1000
    rows = a[:, 0] / 16
    assert np.array_equal(rows, np.sort(rows)) and np.array_equal(a, big[rows.astype(int)].astype(np.float32))
    bench.dump_outputs(str(tmp_path / "c"), {"small": small})               # under the cap: everything, as it was
    assert np.array_equal(np.load(tmp_path / "c" / "small.npy"), small)
