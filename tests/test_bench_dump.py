"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as float64 .npy files (64-bit words as
exact 32-bit halves), at most 64 MB, the same files for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def words_of(halves):
    h = np.asarray(halves)
    assert h.dtype == np.float64 and h.shape[-1] == 2 and (h == np.floor(h)).all() and (h >= 0).all() and (h < 2 ** 32).all()
    return (h[..., 1].astype(np.uint64) << np.uint64(32)) | h[..., 0].astype(np.uint64)


def test_halves_are_exact():
    a = np.array([0, 1, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1, 0x73EDA753299D7D48], dtype=np.uint64)
    assert (words_of(bench.u64_halves(a)) == a).all()


def test_root_words_are_low_limb_first(tmp_path):
    limbs = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x1111111122222222, 0x73EDA753299D7D48]
    root_hex = "".join("%016x" % v for v in reversed(limbs))          # as bench.py's merkle record prints a root
    assert bench.hex_words(root_hex) == limbs
    bench.dump_words(str(tmp_path), "root", bench.hex_words(root_hex))
    assert words_of(np.load(tmp_path / "root.npy")).tolist() == limbs


def test_state_sample_is_fixed_and_within_budget(tmp_path):
    import torch
    n = 1 << 18
    states = torch.arange(n * 20, dtype=torch.int64).view(n, 5, 4)
    for d in ("a", "b"):
        bench.dump_states(str(tmp_path / d), states, 7, 0, 1)
    idx = np.load(tmp_path / "a" / "state_index.npy")
    assert (idx == np.load(tmp_path / "b" / "state_index.npy")).all()
    assert idx.size < n and (np.diff(idx) > 0).all() and idx[0] >= 7 and idx[-1] < n + 7
    got = words_of(np.load(tmp_path / "a" / "states.npy"))
    assert got.shape == (idx.size, 5, 4) and (got[:, 0, 0] == (idx.astype(np.uint64) - np.uint64(7)) * np.uint64(20)).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    small = torch.arange(100 * 20, dtype=torch.int64).view(100, 5, 4)
    bench.dump_states(str(tmp_path / "c"), small, 300, 3, 4)        # a rank's own files; all of a small shard
    assert sorted(os.listdir(tmp_path / "c")) == ["state_index_rank3.npy", "states_rank3.npy"]
    assert (np.load(tmp_path / "c" / "state_index_rank3.npy") == np.arange(300, 400)).all()


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_step_and_repeats(torch_cuda, hades_lib, oracle, tmp_path):
    """Two runs with the same arguments dump the same files; the dumped states are the oracle's permutation applied once per
    launch (parity launch + warm-up + timed steps) to the generator-B inputs of their indices; the digest is the line's."""
    args = ["--steps", "2", "--warmup", "1", "--perms-per-gpu", str(1 << 20), "--no-secondary", "--no-cpu-baseline"]
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py"] + args + ["--dump-outputs", str(tmp_path / d)], cwd=ROOT,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0]))
    assert outs[0]["steps"] == 2 and outs[0]["ms_per_step"] > 0 and outs[0]["digest"] == outs[1]["digest"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["digest.npy", "state_index.npy", "states.npy"] and sorted(os.listdir(tmp_path / "b")) == files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert ["%016x" % int(w) for w in words_of(np.load(tmp_path / "a" / "digest.npy"))] == outs[0]["digest"]
    idx = np.load(tmp_path / "a" / "state_index.npy").astype(np.int64)
    got = words_of(np.load(tmp_path / "a" / "states.npy")).reshape(-1, 20)
    assert idx.size == got.shape[0] > 4096
    pick = np.linspace(0, idx.size - 1, 1024).astype(np.int64)
    exp = np.concatenate([oracle.gen_b(5 * int(i), 5) for i in idx[pick]])
    for _ in range(1 + 1 + 2):
        exp = oracle.perm_batch(exp)
    assert (got[pick].reshape(-1) == exp).all()


@pytest.mark.gpu
def test_bench_merkle_dump_is_the_root_of_the_line(torch_cuda, hades_lib, kat, tmp_path):
    """--workload merkle: root.npy holds the root the line reports, which is the CPU oracle's committed root."""
    r = subprocess.run([sys.executable, "bench.py", "--workload", "merkle", "--steps", "2", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["steps"] == 2 and out["root_matches_golden"] is True and os.listdir(tmp_path) == ["root.npy"]
    root = words_of(np.load(tmp_path / "root.npy")).tolist()
    assert sum(int(v) << (64 * k) for k, v in enumerate(root)) == int(kat["merkle4_full_size"][str(1 << 24)]["root"], 16)
    assert "".join("%016x" % v for v in reversed(root)) == out["root"]
