"""dnrp_rx_sync_batch's tranche schedule (csrc/host/sync.cpp sync_tranches, reported by
dnrp_query_table "sync_tranches"): host logic, no GPU. The frontiers are a function of the sync
geometry (n_steps, step, stf_len) and the launch geometry (n, n_ant) only; DNRP_SYNC_TRANCHE
overrides them."""
import pytest

import dnrp


def _q(*a):
    return [int(f) for f in dnrp.query_table("sync_tranches", *a)]


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("DNRP_SYNC_TRANCHE", raising=False)


def test_default_schedule():
    # the bench's C4 / C3 searches: 1440 steps of 64, stf_len 2304 -> first tranche 4 STFs = 144 steps,
    # then doubling, 4 tranches
    assert _q(1440, 64, 2304, 16384, 4) == [144, 432, 1008, 1440]
    assert _q(1440, 64, 2304, 16384, 1) == [144, 432, 1008, 1440]
    # small batch (under 2^28 DECT samples of step sums): one tranche
    assert _q(1440, 64, 2304, 8, 4) == [1440]
    assert _q(1440, 64, 2304, 728, 4) == [1440] and _q(1440, 64, 2304, 729, 4) == [144, 432, 1008, 1440]
    # short search (under 6 first tranches): one tranche whatever the batch -- C2: 4-sample steps, stf_len 112
    assert _q(400, 4, 112, 1 << 20, 1) == [400]
    assert _q(202, 64, 2304, 1 << 20, 4) == [202]
    assert _q(863, 64, 2304, 1 << 16, 4) == [863] and _q(864, 64, 2304, 1 << 16, 4) == [144, 432, 864]
    # a remainder shorter than the first tranche joins the tranche before it
    assert _q(1100, 64, 2304, 1 << 16, 4) == [144, 432, 1100]
    assert _q(1152, 64, 2304, 1 << 16, 4) == [144, 432, 1008, 1152]
    for n_steps in range(864, 3000, 37):
        fr = _q(n_steps, 64, 2304, 1 << 16, 4)
        assert fr[-1] == n_steps and len(fr) <= 4 and all(b - a >= 144 for a, b in zip([0] + fr, fr)), fr


def test_switch(monkeypatch):
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "0")
    assert _q(1440, 64, 2304, 16384, 4) == [1440]
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "32,64")
    assert _q(202, 64, 2304, 6, 4) == [32, 96, 202]
    assert _q(1440, 64, 2304, 16384, 4) == [32, 96, 1440]
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "150")
    assert _q(202, 4, 112, 6, 1) == [150, 202]
    # sizes that do not fit are dropped: the last tranche takes the rest
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "150,100,20")
    assert _q(202, 4, 112, 6, 1) == [150, 170, 202]
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "202")
    assert _q(202, 4, 112, 6, 1) == [202]
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "")
    assert _q(1440, 64, 2304, 16384, 4) == [1440]


def test_arguments():
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("sync_tranches", 0, 64, 2304, 1, 1)
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("sync_tranches", 1440, 64, 2304, 1)
