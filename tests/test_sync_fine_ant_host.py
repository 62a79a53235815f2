"""Fine search over every antenna with a coarse peak, host side (no GPU): the argument checks of
dnrp_ctx_set_sync_fine_all_antennas / dnrp_ctx_get_sync_fine_all_antennas / dnrp_rx_sync_fine_peaks that need
no context (the round trip runs on a context in tests/test_gpu_sync_fine_ant.py: a context opens the device),
and the margin proof of the inputs the GPU file uses: at the oracle's coarse peak the search restated in numpy
(tests/sync_fine_ant_cases.py) has, on every committed window, a best lag and a best template so far ahead of
the others that the GPU file may demand exact indices and an exact N_eff_TX.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import sync_fine_ant_cases as A

dnrp = pytest.importorskip("dnrp")

EINVAL = -1
MARGIN = 2 * A.RTOL_METRIC  # two metrics each within RTOL_METRIC of the restatement keep their order

INPUTS = [(c, None) for c in A.CASES] + [(A.FOUR, v) for v in sorted(A.VARIANTS)]


def _id(p):
    return A.case_id(p[0]) + ("_" + p[1] if p[1] else "")


def test_null_context():
    L = dnrp.lib()
    on = C.c_uint32(7)
    for v in (0, 1, 2):
        assert L.dnrp_ctx_set_sync_fine_all_antennas(None, v) == EINVAL, v
    assert L.dnrp_ctx_get_sync_fine_all_antennas(None, C.byref(on)) == EINVAL
    assert on.value == 7  # nothing written on an error
    m, i = np.full((1, 8, 4), 7, np.float32), np.full((1, 8, 4), 7, np.uint32)
    assert L.dnrp_rx_sync_fine_peaks(None, 1, C.c_void_p(m.ctypes.data), C.c_void_p(i.ctypes.data), None) == EINVAL
    assert (m == 7).all() and (i == 7).all()
    for name in ("set_sync_fine_all_antennas", "sync_fine_all_antennas", "sync_fine_peaks"):
        assert hasattr(dnrp.Phy, name), name


def _oracle_peaks(c, win):
    ref = O.sync(A.oracle_sync_cfg(c), win, max_reports=1)
    assert len(ref) == 1
    o = ref[0]
    return o, A.antenna_peaks(win, c, o["coarse_64"], o["cfo_frac"], o["coarse_metric"])


@pytest.mark.parametrize("p", INPUTS, ids=_id)
def test_inputs_have_margin(p):
    """A condition on the inputs of tests/test_gpu_sync_fine_ant.py, not a measurement of the library. For every
    (window, processed antenna, template) the restated |xcorr| at the best lag exceeds every other lag's by the
    relative margin 2 RTOL_METRIC, and for every window the largest metric sum exceeds the second largest by
    the same margin: a device metric within RTOL_METRIC of the restatement then has the same argmax."""
    c, variant = p
    nt = A.sync_geometry(c)["n_templates"]
    for w, (win, start, _, delays) in enumerate(A.windows(c, variant)):
        o, (metric, index, xc) = _oracle_peaks(c, win)
        processed = sorted(xc)
        silent = A.VARIANTS[variant]["silent"] if variant else None
        assert processed == [a for a in range(c[5]) if a != silent], (w, processed, o["coarse_metric"])
        for a in processed:
            for k in range(nt):
                r = xc[a][k].copy()
                best = r[index[a, k]]
                r[index[a, k]] = 0.0
                print(_id(p), "window", w, "antenna", a, "template", k, "lag margin", 1 - r.max() / best)
                assert r.max() <= best * (1 - MARGIN), (w, a, k, r.max() / best)
        ms, x, k_likely = A.combine(metric, index, o["coarse_metric"], nt)
        rest = np.delete(ms, k_likely)
        if len(rest):
            print(_id(p), "window", w, "sum margin", 1 - rest.max() / ms[k_likely])
            assert rest.max() <= ms[k_likely] * (1 - MARGIN), (w, ms)
        assert 1 << k_likely == O.packet_sizes(O.psdef(*A.psdef(c)))["N_eff_TX"], (w, ms)
        # the per-antenna peaks of the transmitted template sit at the antennas' own starts
        base = o["coarse_64"] - A.sync_geometry(c)["xc_l"]
        assert [base + int(index[a, k_likely]) for a in processed] == [start + delays[a] for a in processed], w


def test_variant_c_on_differs_from_off():
    """variant (c): the antenna with the largest coarse metric is the one delayed by 3 hw samples, so the fine
    peak of the strongest antenna alone (setting off) and the metric-weighted mean (setting on) differ; the mean
    lies at least 0.05 from a half-integer, so its rounding is not in question."""
    c = A.FOUR
    nt = A.sync_geometry(c)["n_templates"]
    for win, start, _, delays in A.windows(c, "c"):
        o, (metric, index, _) = _oracle_peaks(c, win)
        s = A.strongest(o["coarse_metric"], c[5])
        assert delays[s] == max(delays) == 3, (s, o["coarse_metric"])
        _, x, k_on = A.combine(metric, index, o["coarse_metric"], nt)
        k_off = int(np.argmax(metric[s, :nt]))
        off = int(index[s, k_off])
        assert abs(x[k_on] - np.floor(x[k_on]) - 0.5) >= 0.05, x
        on = int(np.round(x[k_on]))
        base = o["coarse_64"] - A.sync_geometry(c)["xc_l"]
        print("variant c: off", base + off, "on", base + on, "x", x[k_on], "start", start)
        assert base + off == start + 3 and on != off and start <= base + on < start + 3


def test_beta_inputs_have_margin():
    """the windows of test_with_the_beta_search: the same two conditions against the b = 1 template rows, at the
    coarse peak of the oracle search of the packet's own b"""
    cb = A.BETA_CASE
    c, nt = cb[:7], A.sync_geometry(cb[:7])["n_templates"]
    for w, (win, start, _, _) in enumerate(A.K.windows(cb)):
        ref = O.sync(A.K.oracle_sync_cfg(cb), win, max_reports=1)
        assert len(ref) == 1 and ref[0]["fine_64"] == start
        o = ref[0]
        metric, index, xc = A.antenna_peaks(win, c, o["coarse_64"], o["cfo_frac"], o["coarse_metric"], b=cb[7])
        assert sorted(xc) == [0, 1]
        for a in xc:
            for k in range(nt):
                r = xc[a][k].copy()
                best = r[index[a, k]]
                r[index[a, k]] = 0.0
                print("beta window", w, "antenna", a, "template", k, "lag margin", 1 - r.max() / best)
                assert r.max() <= best * (1 - MARGIN), (w, a, k, r.max() / best)
        ms, _, k_likely = A.combine(metric, index, o["coarse_metric"], nt)
        assert np.delete(ms, k_likely).max() <= ms[k_likely] * (1 - MARGIN), (w, ms)
        assert 1 << k_likely == O.packet_sizes(O.psdef(*A.K.psdef(cb)))["N_eff_TX"]


def test_stream_inputs():
    """the two-packet window of test_stream: the oracle search finds both packets at their starts"""
    c = A.CASES[0]
    win, starts = A.two_packet_window(c)
    u, b_max, os_min, L, M, n_ant, _ = c
    osc = O.sync_cfg(u, b_max, os_min=os_min, L=L, M=M, n_ant=n_ant, chunk_len=win.shape[1] * 7 // 8)
    ref = O.sync(osc, win, max_reports=2)
    assert [o["fine_64"] for o in ref] == starts
