"""Residual CFO tracking from the DRS symbols, the parts that need no GPU: the inputs of
tests/test_gpu_rx_cfo_track.py proven against the injected truth (tests/cfo_track_cases.py), the unchanged
oracle on an offset window in l mode (the baseline the GPU benefit test needs), and the error codes of
dnrp_ctx_set_rx_cfo_tracking / dnrp_ctx_get_rx_cfo_tracking / dnrp_rx_cfo_track that need no device.
"""
import ctypes as C

import numpy as np
import pytest

import dnrp
import cfo_track_cases as CT
import oracle_py as O

EINVAL = -1


def _oracle(name, w=None):
    g = CT.geometry(name)
    w = w or CT.window(name)
    return g, w, O.rx(g["ocf"], g["ops"], w["win"], w["off"], 0.0, w["nid"], w["pt"])


def _model(g, w, r, gain=1.0):
    return CT.model_table(g, w["win"], w["off"], 0.0, r["cfo_fine"], CT.inc_of_sto(g, r["sto"]), gain)


@pytest.mark.parametrize("name", CT.MODEL_CASES)
def test_model_against_truth(name):
    """The model's increment follows the injected offset: behind the second op of every stream set, and behind
    every later one, it is the truth inc1 - omega to within the recorded share of omega, which is below the
    20 % cap -- a bound built on the model notices a missing update (all of omega off)."""
    g, w, r = _oracle(name)
    assert g["rot"] <= np.pi / 2 and abs(g["omega"] * g["step"] * g["sym"] - g["rot"]) < 1e-12
    assert len(CT.updates(g)) >= 1 and min(sum(1 for d in g["drs"] if d[1] == tf) for tf in {d[1] for d in g["drs"]}) >= 2
    tab = _model(g, w, r)
    first, dev = CT.first_deviation(g, tab, r["cfo_fine"]), CT.model_deviation(g, tab, r["cfo_fine"])
    print(f"{name}: omega {g['omega']:.4e} rad/sample, {g['rot']} rad per period; model - truth after the second op "
          f"{first:.4f}, largest {dev:.4f} of omega")
    assert first <= CT.MODEL_DEV_FIRST[name] <= CT.DEV_CAP, (name, first)
    assert first <= dev <= CT.MODEL_DEV[name] < CT.DEV_CAP, (name, dev)
    assert np.all(np.isfinite(tab))
    # the STF sees no offset: the entry without an update is the STF's, far below omega
    assert tuple(tab[0]) == tuple(tab[1]) == (0.0, r["cfo_fine"]) and abs(r["cfo_fine"]) < 1e-3 * g["omega"]
    # the phase is continuous at the first CP sample of the symbol behind every DRS symbol
    for l, _, _, _ in g["drs"]:
        if l + 1 <= g["N_DF"]:
            m = l * g["sym"]
            assert abs((tab[l, 0] + m * tab[l, 1]) - (tab[l + 1, 0] + m * tab[l + 1, 1])) < 1e-9, l


def test_model_gain():
    """gain 0: every entry is the STF's and misses the truth by all of omega; gain 0.5: the first update removes
    half of the offset."""
    g, w, r = _oracle("a")
    t0 = _model(g, w, r, gain=0.0)
    assert np.all(t0[:, 0] == 0.0) and np.all(t0[:, 1] == r["cfo_fine"])
    assert CT.model_deviation(g, t0, r["cfo_fine"]) > 0.99
    t5 = _model(g, w, r, gain=0.5)
    l = CT.updates(g)[0]
    assert abs(t5[l + 1, 1] - (r["cfo_fine"] - 0.5 * g["omega"])) < CT.DEV_CAP * g["omega"]


def test_prerotate():
    """The STF entries leave the window as it is; the model's table turns sample m of every symbol behind the
    first update by the table phase less the STF-only phase."""
    g, w, r = _oracle("a")
    flat = np.tile(np.array([0.0, r["cfo_fine"]]), (g["N_DF"] + 1, 1))
    assert np.array_equal(CT.prerotate(g, w["win"], w["off"], flat), w["win"])
    tab = _model(g, w, r)
    pre = CT.prerotate(g, w["win"], w["off"], tab).astype(np.complex128)
    l0 = CT.updates(g)[0]
    for l in (1, l0, l0 + 1, g["N_DF"]):
        m = (l - 1) * g["sym"] + g["CP"] + 7  # m - n_stf of a sample in the transform window
        s = w["off"] + g["n_stf"] + m
        want = np.exp(1j * ((tab[l, 0] - tab[1, 0]) + m * (tab[l, 1] - tab[1, 1])))
        assert abs(pre[0, s] - w["win"][0, s] * want) < 1e-5 * abs(w["win"][0, s]) + 1e-9, l
        assert (tuple(tab[l]) == tuple(tab[1])) == (l <= l0)
    # with the model's table the oracle sees almost no offset behind the second update
    r2 = O.rx(g["ocf"], g["ops"], pre.astype(np.complex64), w["off"], 0.0, w["nid"], w["pt"])
    assert CT.last_quarter_errors(g, w, r2["pdc_llr"]) == 0.0


def test_oracle_without_tracking():
    """Today's receiver on case d's window (l mode: the channel is held from the latest DRS symbol, so the data
    symbols behind it carry the whole residual): the share of wrong PDC signs in the packet's last quarter is
    the recorded baseline, visibly bad, and the model's table removes it."""
    g, w, r = _oracle("d")
    assert g["lr"] == 0
    share = CT.last_quarter_errors(g, w, r["pdc_llr"])
    print(f"oracle without tracking, case d, {g['rot']} rad per period: {share:.4f} of the last quarter's PDC signs wrong")
    assert share >= CT.BASELINE_MIN
    assert abs(share - CT.BASELINE_D) <= 5e-4  # the recorded value (4 decimals)
    pre = CT.prerotate(g, w["win"], w["off"], _model(g, w, r))
    r2 = O.rx(g["ocf"], g["ops"], pre, w["off"], 0.0, w["nid"], w["pt"])
    assert CT.last_quarter_errors(g, w, r2["pdc_llr"]) == 0.0


def test_setter_errors_without_device():
    L = dnrp.lib()
    on, gain, n_sym = C.c_uint32(7), C.c_float(7.0), C.c_uint32(7)
    for o, gn in ((0, 1.0), (1, 1.0), (1, 0.0), (1, float("nan")), (1, float("inf")), (1, -0.5), (1, 1.5), (2, 1.0)):
        assert L.dnrp_ctx_set_rx_cfo_tracking(None, o, gn) == EINVAL, (o, gn)
    assert L.dnrp_ctx_get_rx_cfo_tracking(None, C.byref(on), C.byref(gain)) == EINVAL
    inc, ph = np.zeros(8), np.zeros(8)
    assert L.dnrp_rx_cfo_track(None, 1, C.c_void_p(inc.ctypes.data), C.c_void_p(ph.ctypes.data), 8, C.byref(n_sym),
                               None) == EINVAL
    assert (on.value, gain.value, n_sym.value) == (7, 7.0, 7) and np.all(inc == 0) and np.all(ph == 0)
    for name in ("set_rx_cfo_tracking", "rx_cfo_tracking", "rx_cfo_track"):
        assert callable(getattr(dnrp.Phy, name))
