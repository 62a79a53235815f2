"""CPU checks of the Wiener-LUT parity inputs (tests/lut_cases.py), from the oracle alone: the windows the
GPU parity tests run (tests/test_gpu_parity.py test_rx_lut_*) reach every profile, change the pick inside
a packet where they claim to, stay clear of the pick boundaries, are well conditioned for a float32
pipeline -- and the int16 LLR gate (tests/llr_gate.py) sees a receiver that picks wrongly on them.
Without these a green GPU case would prove nothing about the pick.
"""
import numpy as np
import pytest

import llr_gate
import lut_cases as LC

PACKETS = [(t, i) for t in ("C4", "C3") for i in range(len(LC.TABLES[t][1]))]
MODES = [1, 0]  # chestim_mode_lr: lr, l


def _id(v):
    return {1: "lr", 0: "l"}.get(v, str(v)) if isinstance(v, int) else "-".join(map(str, v))


@pytest.mark.parametrize("lr", MODES, ids=_id)
@pytest.mark.parametrize("pkt", PACKETS, ids=_id)
def test_pick_pattern_and_clearance(pkt, lr):
    """The pick sequence is the table's pattern, both profiles of a step packet at least twice, and every
    estimate at a pick lies 2 dB or more from 5 dB and from 25 dB."""
    t, i = pkt
    LC.check_picks((t, i, lr), LC.oracle(t, i, lr)["lut_picks"], LC.windows(t)[i]["expect"])


def test_tables_reach_every_profile_and_both_steps():
    for t, n in (("C4", 5), ("C3", 4)):
        ws = LC.windows(t)
        assert len(ws) == n
        assert {w["expect"] for w in ws} >= {(0,), (1,), (2,), (2, 1)}
    assert (1, 0) in {w["expect"] for w in LC.windows("C4")}


@pytest.mark.parametrize("lr", MODES, ids=_id)
@pytest.mark.parametrize("pkt", PACKETS, ids=_id)
def test_rows_conditioned_for_float32(pkt, lr):
    """The oracle's float path against its double path: max |delta| <= 1 on PCC and PDC, so a float32
    receiver can meet the +-1 gate on these rows."""
    t, i = pkt
    r, rf = LC.oracle(t, i, lr), LC.oracle(t, i, lr, use_float=True)
    for k in ("pcc_llr", "pdc_llr"):
        d = np.abs(r[k].astype(np.int32) - rf[k].astype(np.int32))
        assert d.max() <= 1, (t, i, lr, k, int(d.max()))
    assert [p for p, _ in rf["lut_picks"]] == [p for p, _ in r["lut_picks"]]


def _mutations(t, i):
    expect = LC.windows(t)[i]["expect"]
    if len(expect) == 2:
        return [dict(pick_stale=True)]
    return [dict(pick_force=p) for p in range(3) if p != expect[0]]


@pytest.mark.parametrize("lr", MODES, ids=_id)
@pytest.mark.parametrize("pkt", PACKETS, ids=_id)
def test_gate_sees_a_wrong_pick(pkt, lr):
    """A receiver that uses the previous DRS operation's pick (step packets) or one wrong profile
    throughout (flat packets) fails the gate against the true oracle on the PDC row."""
    t, i = pkt
    r = LC.oracle(t, i, lr)
    for m in _mutations(t, i):
        rm = LC.oracle(t, i, lr, **m)
        assert rm["lut_picks"] == r["lut_picks"]  # the trace reports the estimate's own pick
        with pytest.raises(AssertionError):
            llr_gate.check(("mutant", t, i, lr, m), rm["pdc_llr"], r["pdc_llr"])
        d = rm["pdc_llr"].astype(np.int32) - r["pdc_llr"].astype(np.int32)
        assert np.count_nonzero(d) / len(d) > 5 * llr_gate.FRAC_MAX, (t, i, lr, m, np.count_nonzero(d) / len(d))


def test_mutations_are_identity_without_a_change():
    """The overrides do nothing else: forcing the profile the estimate picks anyway, or stale-by-one on a
    packet whose pick never changes, reproduces the true oracle bit for bit."""
    r = LC.oracle("C3", 1)
    for m in (dict(pick_force=1), dict(pick_stale=True)):
        rm = LC.oracle("C3", 1, **m)
        assert np.array_equal(rm["pdc_llr"], r["pdc_llr"]) and np.array_equal(rm["pcc_llr"], r["pcc_llr"])


def _sign_consistent(tag, r):
    for k in ("pcc_llr", "pdc_llr"):
        f, q = r[k + "_f"], r[k].astype(np.int32)
        big = np.abs(f) >= 1
        bad = np.flatnonzero(big & ((f > 0) != (q > 0)))
        assert bad.size == 0, (tag, k, bad[:4].tolist(), f[bad[:4]].tolist(), q[bad[:4]].tolist())


@pytest.mark.parametrize("lr", MODES, ids=_id)
@pytest.mark.parametrize("pkt", PACKETS + [("C3_clamp", 0)], ids=_id)
def test_int16_never_opposes_its_float(pkt, lr):
    """The oracle's int16 LLR never has the opposite sign from its own pre-quantisation value where that
    is >= 1 in magnitude: the descrambling negation saturates, -(-32768) = +32767."""
    t, i = pkt
    _sign_consistent((t, i, lr), LC.oracle(t, i, lr))
    _sign_consistent((t, i, lr, "float"), LC.oracle(t, i, lr, use_float=True))


def test_clamp_input_saturates_both_ways():
    """The clamp packet (C3, 12 dB, noise step at -8 dB): picks 1...1 then 0...0 clear of the boundaries,
    at least 16 LLRs past twice full scale of each sign, and int16 full scale of both signs on the row."""
    r = LC.oracle("C3_clamp", 0)
    LC.check_picks("C3_clamp", r["lut_picks"], (1, 0))
    f, q = r["pdc_llr_f"], r["pdc_llr"]
    assert np.count_nonzero(f >= 65536) >= 16 and np.count_nonzero(f <= -65536) >= 16
    assert np.all(q[f >= 65536] == 32767)
    assert np.all(q[f <= -65536] <= -32767)  # quantise, then descramble: -32768, or -(+32767)
    assert np.count_nonzero(q == -32768) > 0 and np.count_nonzero(q == -32767) > 0
