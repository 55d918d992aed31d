"""bench.py's command line, as far as it can be checked without a GPU: the options a plain and a
full run take, and the `--dump-outputs` writer (float32, bounded, the same sample in every run)."""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_writes_the_proof_bytes(tmp_path):
    import bench
    proof = hashlib.shake_256(b"dump").digest(100_003)
    bench.dump_outputs(str(tmp_path / "d"), proof, 0, 1)
    a = np.load(tmp_path / "d" / "proof_bytes.npy")
    assert a.dtype == np.float32 and a.shape == (len(proof),)
    assert a.astype(np.uint8).tobytes() == proof
    n = np.load(tmp_path / "d" / "proof_len.npy")
    assert n.dtype == np.float64 and n.tolist() == [len(proof)]
    # one file pair per rank when several ranks prove
    bench.dump_outputs(str(tmp_path / "d"), proof, 1, 2)
    assert (tmp_path / "d" / "proof_bytes_rank1.npy").exists()


def test_dump_outputs_samples_a_long_proof_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_MAX_VALUES * 4 + 8 <= 64 * 10**6  # float32 values + the length: inside 64 MB
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    proof = hashlib.shake_256(b"long").digest(4099)
    bench.dump_outputs(str(tmp_path / "a"), proof, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), proof, 0, 1)
    a, b = np.load(tmp_path / "a" / "proof_bytes.npy"), np.load(tmp_path / "b" / "proof_bytes.npy")
    assert a.shape == (1000,) and a.dtype == np.float32 and np.array_equal(a, b)
    # the sample is the proof's bytes at sorted, distinct positions: a subsequence of the proof
    it = iter(proof)
    assert all(v in it for v in a.astype(np.uint8).tolist())
    assert np.load(tmp_path / "a" / "proof_len.npy").tolist() == [4099]
