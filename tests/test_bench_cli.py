"""bench.py's command line without a GPU: a plain run is the headline alone, --full brings back every leg, and
--dump-outputs writes float arrays of a fixed size from a fixed sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_headline_and_full_keeps_every_leg(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert a.steps == 7 and a.warmup == 2 and a.lean and a.dump_outputs is None
    for k in ("no_cpu_baseline", "no_cpu_reference", "no_shim", "no_as_shipped", "no_closed_loop", "no_rand64", "no_host_path",
              "no_other_workloads", "no_mixes", "no_exchange_leg", "no_pass_1m", "no_inputs_ready"):
        assert getattr(a, k), k
    f = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "out"], monkeypatch)
    assert not f.lean and f.legs == "all" and f.dump_outputs == "out"
    for k in ("no_cpu_baseline", "no_closed_loop", "no_rand64", "no_host_path", "no_other_workloads", "no_exchange_leg"):
        assert not getattr(f, k), k


def test_dump_messages_writes_a_fixed_sample_as_floats(tmp_path):
    msg = 55
    rng = np.random.default_rng(3)
    parts = [(b, s, rng.integers(0, 256, 30_000 * msg, dtype=np.uint8)) for b in range(2) for s in range(3)]
    for d in ("a", "b"):
        bench.dump_messages(str(tmp_path / d), parts, msg)
    total = 0
    for name in ("replies", "reply_index", "reply_sums"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    rep, idx, sums = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("replies", "reply_index", "reply_sums"))
    assert rep.shape == (bench.DUMP_SAMPLE, msg) and idx.shape == (bench.DUMP_SAMPLE, 3)
    for row, (b, s, i) in zip(rep[::997], idx[::997].astype(int)):  # every sampled row is the message it names
        assert np.array_equal(row, parts[3 * b + s][2].reshape(-1, msg)[i])
    assert sums.shape == (6, 5) and sums[0, 3] == float(parts[0][2].astype(np.int64).sum())
