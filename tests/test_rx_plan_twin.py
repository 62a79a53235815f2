"""The PDC phase's back-end plan with twin segments (geometry.cpp build_rx_plan / split_twins, read
through dnrp_query_table "rx_plan_segs", "rx_plan_epochs", "pdc_cells"): host logic, no GPU.

A twin segment is two consecutive symbols of one interpolation event whose PDC cells sit on the same
subcarrier list; the epoch receiver interpolates a stream's channel once for both. Checked against the
plain plan (twin = 0: the merged segments the Y path keeps) at beta = 1 (28 SFBC pairs per full symbol,
4 mod 6 as at beta = 16), for lr mode with stride 1, 2, 3 and l mode, N_eff_TX 1, 2, 4:
every PDC cell covered exactly once, twins only where both symbols share event and subcarrier list,
none in the full processing stages at stride 1, unit totals consistent.
"""
import numpy as np
import pytest

import dnrp

B = 1
N_DFS = (19, 21, 29, 34)  # 21: the packet ends on a full processing stage, the others have symbols behind it
MODES = [(1, 1), (1, 2), (1, 3), (0, 2)]  # (mode_lr, stride)
SEG = ["epoch", "kind", "l", "j0", "j1", "mode", "rel", "swap", "off", "drs_cnt", "u0", "twin"]


def _plan(nt, n_df, lr, stride, twin):
    a = (B, nt, nt, n_df, lr, stride, twin)
    segs = dnrp.query_table("rx_plan_segs", *a).astype(np.int64).reshape(-1, len(SEG))
    eps = dnrp.query_table("rx_plan_epochs", *a).astype(np.int64).reshape(-1, 3)
    return [dict(zip(SEG, r)) for r in segs], eps


def _cells(nt, n_df):
    c = dnrp.query_table("pdc_cells", B, nt, nt, n_df).astype(np.int64).reshape(-1, 2)
    return c[:, 0], c[:, 1]  # symbol, subcarrier index per cell


@pytest.mark.parametrize("lr,stride", MODES)
@pytest.mark.parametrize("nt", [1, 2, 4])
@pytest.mark.parametrize("n_df", N_DFS)
def test_twin_plan(nt, n_df, lr, stride):
    sym, kk = _cells(nt, n_df)
    per_unit = 2 if nt > 1 else 1
    plain, eps0 = _plan(nt, n_df, lr, stride, 0)
    twin, eps1 = _plan(nt, n_df, lr, stride, 1)
    assert all(s["twin"] == 0 for s in plain)
    assert len(eps0) == len(eps1)

    # every PDC cell exactly once, in both plans, and the same cells per epoch
    for segs in (plain, twin):
        cover = np.zeros(len(sym), int)
        for s in segs:
            assert s["kind"] == 4 and s["j0"] < s["j1"]
            cover[s["j0"]:s["j1"]] += 1
        assert np.all(cover == 1), (nt, n_df, lr, stride)
    for e in range(len(eps0)):
        span = lambda segs: sorted((s["j0"], s["j1"]) for s in segs if s["epoch"] == e)
        a, b = span(plain), span(twin)
        assert a[0][0] == b[0][0] and a[-1][1] == b[-1][1]

    # units: per segment, cumulative u0, per epoch; a twin unit stands for a unit of each symbol
    def units(s):
        return (s["twin"] if s["twin"] else s["j1"] - s["j0"]) // per_unit

    for segs, eps in ((plain, eps0), (twin, eps1)):
        for e, (s0, s1, n_units) in enumerate(eps):
            mine = segs[s0:s1]
            assert all(s["epoch"] == e for s in mine)
            u = 0
            for s in mine:
                assert s["u0"] == u
                u += units(s)
            assert u == n_units
    saved = sum(units(s) for s in twin if s["twin"])
    assert eps0[:, 2].sum() - eps1[:, 2].sum() == saved

    # twins: two consecutive symbols inside one plain (merged, single-event) segment, same subcarriers
    n_twin = 0
    for s in twin:
        n = s["twin"]
        parent = [p for p in plain if p["j0"] <= s["j0"] and s["j1"] <= p["j1"]]
        assert len(parent) == 1, "a segment never straddles two events"
        for f in ("mode", "rel", "swap", "off", "drs_cnt", "epoch"):
            assert s[f] == parent[0][f]
        if not n:
            continue
        n_twin += 1
        j0, j1 = s["j0"], s["j1"]
        assert j1 - j0 == 2 * n and n % per_unit == 0
        assert np.all(sym[j0:j0 + n] == s["l"]) and np.all(sym[j0 + n:j1] == s["l"] + 1)
        # the symbols' whole cell lists, so the pair index of a unit's second symbol is that of cell jj + n
        assert np.count_nonzero(sym == s["l"]) == n and np.count_nonzero(sym == s["l"] + 1) == n
        assert np.array_equal(kk[j0:j0 + n], kk[j0 + n:j1])
    # a plain segment of the twin plan holds no two neighbouring symbols that qualify (greedy pairing
    # from the event's first symbol leaves only singles between twins)
    for s in twin:
        if s["twin"]:
            continue
        ls = sorted(set(sym[s["j0"]:s["j1"]]))
        for la, lb in zip(ls, ls[1:]):
            ka, kb = kk[sym == la], kk[sym == lb]
            assert not (lb == la + 1 and np.array_equal(ka, kb)), (nt, n_df, lr, stride, la)
    if lr and stride == 1:
        # an event per symbol in every full processing stage: no twin there. The symbols behind the last
        # full stage (rx_synced.cpp:1112-1163) have events at DRS symbols only, whatever the stride, and
        # pair up; N_DF = 21 ends on a full stage for every N_eff_TX and has no twin at all
        n_step = 5 if nt <= 2 else 10
        last = n_step + 1 + ((n_df - 1) // n_step - 1) * n_step
        assert all(s["l"] > last for s in twin if s["twin"])
        if n_df == 21:
            assert n_twin == 0
    if lr and stride == 2 and n_df >= 29:
        assert n_twin > 0


def test_twin_plan_odd_event():
    """Stride 3: an event of three symbols on one subcarrier list is a twin and a single."""
    sym, kk = _cells(4, 34)
    twin, _ = _plan(4, 34, 1, 3, 1)
    plain, _ = _plan(4, 34, 1, 3, 0)
    hit = False
    for p in plain:
        ls = sorted(set(sym[p["j0"]:p["j1"]]))
        if len(ls) == 3 and all(np.array_equal(kk[sym == ls[0]], kk[sym == l]) for l in ls):
            inside = [s for s in twin if p["j0"] <= s["j0"] and s["j1"] <= p["j1"]]
            assert [bool(s["twin"]) for s in inside] == [True, False]
            hit = True
    assert hit


def test_plan_query_arguments():
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("rx_plan_segs", B, 4, 4, 34, 1, 0, 1)  # stride 0
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("rx_plan_segs", B, 4, 4, 34, 1, 2)
