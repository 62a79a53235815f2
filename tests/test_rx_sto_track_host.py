"""Residual STO tracking from the DRS symbols, the parts that need no GPU: the inputs of
tests/test_gpu_rx_sto_track.py proven against the injected truth (tests/sto_track_cases.py), the oracle
without tracking on a drifted window, and the error codes of dnrp_ctx_set_rx_sto_tracking /
dnrp_ctx_get_rx_sto_tracking / dnrp_rx_sto_track that need no device.

choose_pdc_path (host/rx.cpp) is not behind dnrp_query_table, the host-test hook; that the fused receiver
and the grouped Y path are not taken while tracking is on is checked by launch counts on the GPU
(tests/test_gpu_rx_sto_track.py test_gain0_is_the_old_receiver).
"""
import ctypes as C

import numpy as np
import pytest

import dnrp
import oracle_py as O
import sto_track_cases as ST

EINVAL = -1


def _oracle(name, w=None):
    g = ST.geometry(name)
    w = w or ST.window(name)
    return g, w, O.rx(g["ocf"], g["ops"], w["win"], w["off"], 0.0, w["nid"], w["pt"])


@pytest.mark.parametrize("name", ST.MODEL_CASES)
def test_model_against_truth(name):
    """The model's table follows the injected drift: after every DRS symbol it holds the increment that removes
    the delay accumulated at that symbol, to within the recorded share of one DRS period's drift, which is
    below the 20 % cap -- a bound built on the model notices a missing update (a whole period off)."""
    g, w, r = _oracle(name)
    tab = ST.model_table(g, w["win"], w["off"], ST.inc_of_sto(g, r["sto"]), r["cfo_fine"])
    dev = ST.model_deviation(g, tab)
    last = g["eps"] * g["N_DF"] * (g["CP"] + g["Nd"])
    print(f"{name}: deviation {dev:.4f} of a period's drift ({ST.period_drift(g):.3e} rad), delay at the last "
          f"symbol {last:.2f} of CP {g['CP']} samples")
    assert dev <= ST.MODEL_DEV[name] < ST.DEV_CAP, (name, dev)
    assert last < g["CP"] / 4, (name, last)
    assert np.all(np.isfinite(tab)) and tab[0] == tab[1] == ST.inc_of_sto(g, r["sto"])
    # the STF sees no drift: its estimate is far below one period's drift
    assert abs(tab[0]) < 1e-3 * ST.period_drift(g), (name, tab[0])


def test_model_gain():
    """gain 0: the table is the STF increment and misses the truth by whole periods; gain 0.5: every update is
    half the residual, so the table trails the truth by a known recurrence."""
    g, w, r = _oracle("a")
    inc = ST.inc_of_sto(g, r["sto"])
    t0 = ST.model_table(g, w["win"], w["off"], inc, r["cfo_fine"], gain=0.0)
    assert np.all(t0 == inc)
    assert ST.model_deviation(g, t0) > 1.0
    t5 = ST.model_table(g, w["win"], w["off"], inc, r["cfo_fine"], gain=0.5)
    run = 0.0
    for l, _, _, _ in g["drs"]:
        run += 0.5 * (ST.truth_inc(g, l) - run)
        assert abs(t5[l + 1] - inc - run) < ST.DEV_CAP * ST.period_drift(g), (l, t5[l + 1], run)


def test_prerotate():
    """A table equal to the STF increment leaves the window as it is; the model's table turns the bins of every
    symbol behind the first DRS symbol by exp(j (table - STF increment) k)."""
    g, w, r = _oracle("a")
    inc = ST.inc_of_sto(g, r["sto"])
    flat = np.full(g["N_DF"] + 1, inc)
    assert np.array_equal(ST.prerotate(g, w["win"], w["off"], flat), w["win"])
    tab = ST.model_table(g, w["win"], w["off"], inc, r["cfo_fine"])
    pre = ST.prerotate(g, w["win"], w["off"], tab)
    Nd, ks = g["Nd"], np.fft.fftfreq(g["Nd"], 1.0 / g["Nd"])
    occ = (np.abs(ks) <= g["N"] // 2) & (ks != 0)
    for l in (1, 2, 9, g["N_DF"]):
        m0 = w["off"] + g["n_stf"] + (l - 1) * (g["CP"] + Nd) + g["CP"]
        a, b = np.fft.fft(pre[0, m0:m0 + Nd].astype(np.complex128)), np.fft.fft(w["win"][0, m0:m0 + Nd].astype(np.complex128))
        want = np.exp(1j * (tab[l] - tab[0]) * ks)
        assert np.max(np.abs(a[occ] / b[occ] - want[occ])) < 1e-4, l  # complex64 windows
        assert (tab[l] == tab[0]) == (l == 1)


def test_oracle_without_tracking():
    """Today's receiver on the longest generic drifted window: recorded, not required to fail -- the time
    interpolation between DRS symbols absorbs a linear drift."""
    g, w, r = _oracle("b")
    share = ST.last_quarter_errors(g, w, r["pdc_llr"])
    print(f"oracle without tracking, case b: {share:.4f} of the last quarter's PDC signs wrong")
    assert share < 0.01


def test_setter_errors_without_device():
    L = dnrp.lib()
    on, gain, n_sym = C.c_uint32(7), C.c_float(7.0), C.c_uint32(7)
    for o, gn in ((0, 1.0), (1, 1.0), (1, 0.0), (1, float("nan")), (1, float("inf")), (1, -0.5), (1, 1.5), (2, 1.0)):
        assert L.dnrp_ctx_set_rx_sto_tracking(None, o, gn) == EINVAL, (o, gn)
    assert L.dnrp_ctx_get_rx_sto_tracking(None, C.byref(on), C.byref(gain)) == EINVAL
    inc = np.zeros(8)
    assert L.dnrp_rx_sto_track(None, 1, C.c_void_p(inc.ctypes.data), 8, C.byref(n_sym), None) == EINVAL
    assert (on.value, gain.value, n_sym.value) == (7, 7.0, 7) and np.all(inc == 0)
    for name in ("set_rx_sto_tracking", "rx_sto_tracking", "rx_sto_track"):
        assert callable(getattr(dnrp.Phy, name))
