"""Step sums in tranches (dnrp_rx_sync_batch, DNRP_SYNC_TRANCHE): the step-sum kernels compute a
range of steps, the detection runs up to that frontier, finished windows skip the later tranches.

 - parity against the oracle with forced tranches 32,64 for every step-sum kernel family (pipe,
   single-prefetch stream, wave, step-4 stream, tile, os_min 2) and for the inline / one-round
   detection forms;
 - the detection step on, next to and straddling a tranche boundary: every report field equal to
   the untranched run (detection RMS / metric to 1e-3: a step's partial sums are added in an order
   that depends on its position in its segment, as DNRP_SS_SEG_CHUNKS already moves it);
 - a mixed batch (early, late, none, two packets in different tranches, max_reports 1 and 2), called
   twice on one context with the packets elsewhere: no stale step values or states leak;
 - the default schedule: one tranche for the small test geometries, several for the bench's (the
   schedule itself through dnrp_query_table, the launches through the sync_steps timer count).

Tolerances against the oracle are test_gpu_sync.py's (_compare).
"""
import functools

import numpy as np
import pytest

import oracle_py as O
import phy_fixtures as F
from test_gpu_sync import _compare, _phy, _run

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROUNDING_FIELDS = ("detection_rms", "detection_metric")  # derived from the step sums' float rounding


@functools.lru_cache(maxsize=None)
def _case(name, S_win, chunk, seed=21):
    """5 packet windows + 1 noise window of `name` and the oracle's reports (max_reports = 2), shared
    by every test of that geometry."""
    rng = np.random.default_rng(seed)
    psd, cfgt = F.case(name)
    windows, truth = [], []
    for _ in range(5):
        start = int(rng.integers(0.15 * S_win, 0.3 * S_win))
        cfo = rng.uniform(-1.75, 1.75) * 2 * np.pi / (64 * psd[1] * cfgt[3])
        windows.append(F.sync_window(rng, O, name, S_win, [start], cfo)[0])
        truth.append(start)
    windows.append(F.sync_window(rng, O, name, S_win, [], 0.0)[0])
    osc = O.sync_cfg(psd[0], psd[1], os_min=cfgt[3], L=cfgt[4], M=cfgt[5], n_ant=cfgt[2], chunk_len=chunk)
    refs = [O.sync(osc, w, max_reports=2) for w in windows]
    return windows, truth, refs


def _check_oracle(where, res, cnt, refs, max_reports):
    for w, ref in enumerate(refs):
        ref = ref[:max_reports]
        assert int(cnt[w]) == len(ref), (where, w, int(cnt[w]), len(ref))
        for k, o in enumerate(ref):
            _compare(res[w, k], o, (where, w, k))
        for k in range(len(ref), max_reports):
            assert int(res[w, k]["found"]) == 0, (where, w, k)


def _check_equal(where, res, cnt, res0, cnt0):
    """Tranched against untranched results: counts, found flags and every field of every found report
    identical, the two step-sum-derived fields within rtol 1e-3."""
    assert np.array_equal(cnt, cnt0), (where, cnt, cnt0)
    assert np.array_equal(res["found"], res0["found"]), where
    for w in range(res.shape[0]):
        for k in range(int(cnt[w])):
            for f in res.dtype.names:
                if f in ROUNDING_FIELDS:
                    np.testing.assert_allclose(res[w, k][f], res0[w, k][f], rtol=1e-3, err_msg=str((where, w, k, f)))
                else:
                    assert np.array_equal(res[w, k][f], res0[w, k][f]), (where, w, k, f, res[w, k][f], res0[w, k][f])


def _parity(name, S_win, chunk, phy=None):
    import dnrp
    psd, cfgt = F.case(name)
    windows, truth, refs = _case(name, S_win, chunk)
    phy = phy or _phy(name)
    res, cnt = _run(phy, dnrp.SyncCfg(psd[0], psd[1], cfgt[2], chunk, 2), windows, 2)
    _check_oracle(name, res, cnt, refs, 2)
    for w, start in enumerate(truth):
        assert int(res[w, 0]["fine_peak_time"]) == start, (name, w)
    return res, cnt


PARITY = [
    ("C4", 20480, 4096, {}),                          # sync_steps_pipe_kernel
    ("C4", 20480, 4096, {"DNRP_SYNC_PIPE": "0"}),     # sync_steps_stream_kernel<.., 16, 1>
    ("C4", 20480, 4096, {"DNRP_SYNC_STREAM": "0"}),   # sync_steps_wave_kernel
    ("C2", 1500, 400, {}),                            # sync_steps_stream_kernel<.., 0>, 4-sample steps
    ("lm1_1_u8b16", 20480, 4096, {}),                 # sync_steps_kernel (tiles)
    ("os2_u2b2_tm1", 6000, 1200, {}),                 # sync_steps_kernel<9, 10, 4>
    ("C4", 20480, 4096, {"DNRP_SYNC_ROUNDS": "0"}),   # inline detection alone
    ("C4", 20480, 4096, {"DNRP_SYNC_ROUNDS": "1"}),   # one split round, the rest inline
]


@pytest.mark.parametrize("name,S_win,chunk,env", PARITY)
def test_tranche_parity(name, S_win, chunk, env, monkeypatch):
    """Forced tranches 32,64 (frontiers 32, 96, n_steps ~ 202-212): the packets' detections fall into
    the second and third tranche, the noise window runs through all three."""
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "32,64")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _parity(name, S_win, chunk)


def test_tranche_frontier_boundary(monkeypatch):
    """The detection step sd on the first step of tranche 2 (first tranche of sd steps), on the last
    step of tranche 1 (sd + 1), one step inside it (sd + 2), and with its 36-step history straddling
    the boundary (sd - 17): all as the untranched run."""
    import dnrp
    psd, cfgt = F.case("C4")
    windows, _, _ = _case("C4", 20480, 4096)
    win = [windows[0]]
    phy = _phy("C4")
    sc = dnrp.SyncCfg(psd[0], psd[1], cfgt[2], 4096, 2)
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "0")
    res0, cnt0 = _run(phy, sc, win, 2)
    assert int(cnt0[0]) >= 1
    step = 16 * psd[1] // 4  # pattern / SYNC_STEP_DIVIDER at os_min 1
    sd = int(res0[0, 0]["detection_time_local"]) // step - 1
    assert 36 + 17 < sd < 200, sd
    for first in (sd, sd + 1, sd + 2, sd - 17):
        monkeypatch.setenv("DNRP_SYNC_TRANCHE", str(first))
        res, cnt = _run(phy, sc, win, 2)
        _check_equal(("first tranche", first, "sd", sd), res, cnt, res0, cnt0)


MIXED_STARTS = [[300], [1650], [], [307, 1645], [900], [350], [1600], [320, 1610]]


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(27)
    windows = [F.sync_window(rng, O, "C2", 3000, st, 0.3 * (i - 3) * 2 * np.pi / 64)[0] for i, st in enumerate(MIXED_STARTS)]
    osc = O.sync_cfg(1, 1, n_ant=1, chunk_len=3000)
    return windows, [O.sync(osc, w, max_reports=2) for w in windows]


@pytest.mark.parametrize("rounds", [None, "2"])
@pytest.mark.parametrize("max_reports", [2, 1])
def test_tranche_mixed_batch(max_reports, rounds, monkeypatch):
    """8 C2 windows of 3000 samples (787 steps) in one call, tranches 150,200 (frontiers 150, 350, 787):
    early packets finish in tranche 1, late ones in the last, the noise window runs through all with
    nothing found, two packets in different tranches are both reported with max_reports = 2 and only
    the first with max_reports = 1. Then the same context again with the windows in reverse order:
    step values and states left by the first call must not leak."""
    import dnrp
    if rounds is not None:
        monkeypatch.setenv("DNRP_SYNC_ROUNDS", rounds)
    windows, refs = _mixed()
    assert [len(r) for r in refs] == [len(s) for s in MIXED_STARTS]
    step = 4
    for st, ref in zip(MIXED_STARTS, refs):  # the detections sit in the tranches the test is about
        for s0, o in zip(st, ref):
            sd = o["det_time"] // step - 1
            assert (sd < 150) if s0 < 400 else (150 <= sd < 350) if s0 < 1000 else (sd >= 350), (s0, sd)
    phy = _phy("C2")
    sc = dnrp.SyncCfg(1, 1, 1, 3000, max_reports)
    for order in (slice(None), slice(None, None, -1)):
        wl, rl = windows[order], refs[order]
        monkeypatch.setenv("DNRP_SYNC_TRANCHE", "150,200")
        res, cnt = _run(phy, sc, wl, max_reports)
        _check_oracle(("mixed", max_reports), res, cnt, rl, max_reports)
        assert [int(c) for c in cnt] == [min(len(r), max_reports) for r in rl]
        monkeypatch.setenv("DNRP_SYNC_TRANCHE", "0")
        res0, cnt0 = _run(phy, sc, wl, max_reports)
        _check_equal(("mixed", max_reports), res, cnt, res0, cnt0)


def _steps_launches(phy):
    return phy.kernel_time_total("sync_steps", reset=True)[1]


@pytest.mark.parametrize("name,S_win,chunk,n_steps,step,stf_len", [("C4", 20480, 4096, 202, 64, 2304),
                                                                    ("C2", 1500, 400, 202, 4, 112)])
def test_tranche_default_schedule(name, S_win, chunk, n_steps, step, stf_len, monkeypatch):
    """No switch set: the schedule is a function of the geometry. These short searches of 6 windows
    run as one tranche (one sync_steps launch per call), as the schedule says; forced tranches show in
    the same count."""
    import dnrp
    monkeypatch.delenv("DNRP_SYNC_TRANCHE", raising=False)
    monkeypatch.setenv("DNRP_TIMING", "1")
    n_ant = F.case(name)[1][2]
    want = [int(f) for f in dnrp.query_table("sync_tranches", n_steps, step, stf_len, 6, n_ant)]
    assert want == [n_steps]
    phy = _phy(name)
    _steps_launches(phy)
    _parity(name, S_win, chunk, phy)
    assert _steps_launches(phy) == len(want) == 1
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "32,64")
    _parity(name, S_win, chunk, phy)
    assert _steps_launches(phy) == 3
