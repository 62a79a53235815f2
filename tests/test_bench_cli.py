"""bench.py's command line and --dump-outputs on the CPU (no GPU work): a plain run leaves --full
off, --steps must be a positive count, and dump_outputs writes the float arrays of a fixed sample of
the chunk's slots, the LLR rows looked up through the windows of the last RX pass."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
dnrp = pytest.importorskip("dnrp")

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import bench  # noqa: E402


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs(tmp_path):
    chunk, n_tx, S, G, n_rx = 256, 2, 500, 3000, 2
    rng = np.random.default_rng(3)
    res = np.zeros((chunk, 1), dnrp.SYNC_RESULT_DTYPE)
    res["fine_peak_time"] = 2400 + rng.integers(0, 32, (chunk, 1))
    res["N_eff_TX"] = 4
    res["rms_array"] = rng.random((chunk, 1, 8), dtype=np.float32)
    cnt = np.ones(chunk, np.uint32)
    missed = [5, 77]
    cnt[missed] = 0  # two windows without a packet: their PCC / PDC rows do not exist
    reps = dnrp.found_reports(res, cnt)
    tx = torch.from_numpy(rng.standard_normal((chunk, n_tx, S, 2), dtype=np.float32))
    pcc = torch.from_numpy(rng.integers(-99, 100, (chunk, 196)).astype(np.int16))
    pdc = torch.from_numpy(rng.integers(-999, 1000, (chunk, G)).astype(np.int16))
    # the MAC continued with every second found packet: PDC row j belongs to PCC row 2 j
    state = {"pcc_windows": reps["window"], "pdc_windows": reps["window"][::2]}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), reps, state, tx, pcc, pdc, n_rx)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["pcc_llr", "pdc_llr", "slots", "sync_reports", "sync_rms", "tx_iq"]
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name  # the sample is fixed
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    slots = got["slots"].astype(np.int64)
    assert len(slots) == 64 and (np.diff(slots) > 0).all() and slots.min() >= 0 and slots.max() < chunk
    assert got["sync_reports"].shape == (chunk - 2, 7) and got["sync_rms"].shape == (chunk - 2, n_rx)
    assert np.array_equal(got["sync_reports"][:, 0], reps["window"])
    assert np.array_equal(got["sync_reports"][:, 1], reps["fine_peak_time"])
    assert np.array_equal(got["sync_rms"], reps["rms"][:, :n_rx])
    assert np.array_equal(got["tx_iq"], tx.numpy()[slots])
    pcc_row = {int(w): r for r, w in enumerate(reps["window"])}
    pdc_row = {int(w): r for r, w in enumerate(reps["window"][::2])}
    for i, s in enumerate(slots):
        want = pcc[pcc_row[s]].numpy() if s in pcc_row else np.zeros(196)
        assert np.array_equal(got["pcc_llr"][i], want), s
        want = pdc[pdc_row[s]].numpy() if s in pdc_row else np.zeros(G)
        assert np.array_equal(got["pdc_llr"][i], want), s
