"""Fine search over every antenna with a coarse peak on the GPU (dnrp_ctx_set_sync_fine_all_antennas,
dnrp_rx_sync_fine_peaks; kernels/sync_fine.hip sync_fine_ant_kernel, sync_fine_combine_kernel), inputs and the numpy
restatement of tests/sync_fine_ant_cases.py (tests/test_sync_fine_ant_host.py proves the inputs' margins, which
is what lets this file demand exact indices and an exact N_eff_TX).

1. Setter / getter round trip and the error codes of dnrp_rx_sync_fine_peaks.
2. Off is off: never touched, set to 0, set to 1 and back to 0 give byte-identical reports.
3. On changes only fine_peak_time, fine_peak_time_local, N_eff_TX, fine_peak_metric, fine_peak_index; with one
   searched antenna nothing.
4. The per-antenna table against the restatement: indices exact, metrics within RTOL_METRIC (the tolerance of
   tests/test_gpu_sync.py:54), unprocessed entries 0.
5. The report against the combination of the device's own table computed in numpy.
6. Variant (c): on and off report different fine peaks, each its restatement's; variant (a): the fine peak
   lies within the antennas' true starts.
7. Variant (a) through rx_pcc_batch / rx_pdc_batch: every hard decision is the transmitted bit.
8. With the beta search on as well.  9. Through rx_sync_stream.  10. Twice the same bytes.
"""
import numpy as np
import pytest

import oracle_py as O
import sync_beta_cases as K
import sync_fine_ant_cases as A

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CHANGED = ("fine_peak_time", "fine_peak_time_local", "N_eff_TX", "fine_peak_metric", "fine_peak_index")
INPUTS = [(c, None) for c in A.CASES] + [(A.FOUR, v) for v in sorted(A.VARIANTS)]
MAX_REPORTS = 2  # one packet per window: the second slot of every window is not `found`


def _id(p):
    return A.case_id(p[0]) + ("_" + p[1] if p[1] else "")


def _phy(c, max_batch=8):
    import dnrp
    u, b_max, os_min, L, M, n_ant, _ = c[:7]
    phy = dnrp.Phy(u, b_max, n_ant, os_min, L, M, max_batch=max_batch)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    return phy


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(*a.shape, 2)).to("cuda:0")


def _sync(phy, c, wins, n_lim=None, max_reports=MAX_REPORTS, chunk=None):
    import dnrp
    n, (n_ant, S) = len(wins), wins[0].shape
    sc = dnrp.SyncCfg(c[0], c[1], n_lim or n_ant, chunk or A.chunk_len(c), max_reports)
    res, cnt = phy.rx_sync_batch(sc, _to_dev(np.stack(wins)), n, S, n_ant * S, S)
    phy.sync()
    return res, cnt


def _same(x, y, fields=None):
    """the `found` flags of every slot and the bytes of the fields (default: all) of every found slot"""
    assert np.array_equal(x["found"], y["found"])
    for f in fields or x.dtype.names:
        assert x[f][x["found"] == 1].tobytes() == y[f][y["found"] == 1].tobytes(), f


_RUNS = {}


def _runs(p):
    """One off run and one on run (reports, counts, table) of an input, shared by the tests below and left
    unchanged by them."""
    if p not in _RUNS:
        c, variant = p
        phy = _phy(c)
        wins = [m[0] for m in A.windows(c, variant)]
        off, cnt_off = _sync(phy, c, wins)
        phy.set_sync_fine_all_antennas(1)
        on, cnt_on = _sync(phy, c, wins)
        metric, index = phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
        phy.close()
        _RUNS[p] = dict(off=off, cnt_off=cnt_off, on=on, cnt_on=cnt_on, metric=metric, index=index)
    return _RUNS[p]


def _restated(c, win, r, n_lim=None, b=None):
    """the restatement at the coarse peak, CFO and coarse_peak_array of the report r"""
    return A.antenna_peaks(win, c, int(r["coarse_peak_time"]), float(r["cfo_fractional_rad"]), r["coarse_peak_array"],
                           n_lim=n_lim, b=b)


def test_round_trip_and_states():
    import dnrp
    c = A.CASES[0]
    phy = _phy(c)
    assert phy.sync_fine_all_antennas() is False  # the default
    phy.set_sync_fine_all_antennas(1)
    assert phy.sync_fine_all_antennas() is True
    with pytest.raises(dnrp.DnrpError) as e:
        phy.set_sync_fine_all_antennas(2)
    assert e.value.code == -1 and phy.sync_fine_all_antennas() is True  # a refused call changes nothing
    with pytest.raises(dnrp.DnrpError) as e:  # no sync call yet
        phy.sync_fine_peaks(2)
    assert e.value.code == -7
    wins = [m[0] for m in A.windows(c)]
    _sync(phy, c, wins)
    for bad in (len(wins) * MAX_REPORTS - 1, len(wins) * MAX_REPORTS + 1, 0):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.sync_fine_peaks(bad)
        assert e.value.code == -1, bad
    m, i = phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
    assert m.shape == i.shape == (len(wins) * MAX_REPORTS, 8, 4) and m.dtype == np.float32 and i.dtype == np.uint32
    null = dnrp.lib().dnrp_rx_sync_fine_peaks
    assert null(phy._ctx, len(wins) * MAX_REPORTS, None, i.ctypes.data, None) == -1
    assert null(phy._ctx, len(wins) * MAX_REPORTS, m.ctypes.data, None, None) == -1
    phy.set_sync_fine_all_antennas(0)
    assert phy.sync_fine_all_antennas() is False
    _sync(phy, c, wins)
    with pytest.raises(dnrp.DnrpError) as e:  # the latest sync call ran with the setting off
        phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
    assert e.value.code == -7
    phy.close()


@pytest.mark.parametrize("p", INPUTS, ids=_id)
def test_off_is_off(p):
    c, variant = p
    wins = [m[0] for m in A.windows(c, variant)]
    phy = _phy(c)
    never, cnt0 = _sync(phy, c, wins)
    phy.set_sync_fine_all_antennas(0)
    zero, cnt1 = _sync(phy, c, wins)
    phy.set_sync_fine_all_antennas(1)
    phy.set_sync_fine_all_antennas(0)
    back, cnt2 = _sync(phy, c, wins)
    phy.close()
    assert list(cnt0) == list(cnt1) == list(cnt2) == [1] * len(wins)
    _same(never, zero)
    _same(never, back)
    _same(never, _runs(p)["off"])


@pytest.mark.parametrize("p", INPUTS, ids=_id)
def test_only_the_five_fields_change(p):
    r = _runs(p)
    assert list(r["cnt_on"]) == list(r["cnt_off"]) == [1] * len(r["cnt_on"])
    _same(r["on"], r["off"], [f for f in r["on"].dtype.names if f not in CHANGED])


@pytest.mark.parametrize("c", [A.CASES[0], A.FOUR], ids=A.case_id)
def test_one_searched_antenna_changes_nothing(c):
    wins = [m[0] for m in A.windows(c)]
    phy = _phy(c)
    off, cnt_off = _sync(phy, c, wins, n_lim=1)
    phy.set_sync_fine_all_antennas(1)
    on, cnt_on = _sync(phy, c, wins, n_lim=1)
    metric, index = phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
    phy.close()
    assert list(cnt_on) == list(cnt_off) == [1] * len(wins)
    _same(on, off)
    for w in range(len(wins)):  # the table: the one antenna's row is the report's
        assert metric[w * MAX_REPORTS, 0].tobytes() == on[w, 0]["fine_peak_metric"].tobytes()
        assert index[w * MAX_REPORTS, 0].tobytes() == on[w, 0]["fine_peak_index"].tobytes()
        assert not metric[w * MAX_REPORTS, 1:].any() and not index[w * MAX_REPORTS, 1:].any()


@pytest.mark.parametrize("p", INPUTS, ids=_id)
def test_per_antenna_parity(p):
    c, variant = p
    r, nt = _runs(p), A.sync_geometry(c)["n_templates"]
    worst = 0.0
    for w, (win, _, _, _) in enumerate(A.windows(c, variant)):
        rep = r["on"][w, 0]
        assert int(rep["found"]) == 1 and int(r["on"][w, 1]["found"]) == 0
        metric, index, xc = _restated(c, win, rep)
        got_m, got_i = r["metric"][w * MAX_REPORTS], r["index"][w * MAX_REPORTS]
        assert np.array_equal(got_i, index), (w, got_i, index)
        for a in range(8):
            if a in xc:
                dev = np.abs(got_m[a, :nt] / metric[a, :nt] - 1).max()
                worst = max(worst, dev)
                assert dev <= A.RTOL_METRIC, (w, a, got_m[a], metric[a])
                assert not got_m[a, nt:].any()
            else:
                assert not got_m[a].any() and not got_i[a].any(), (w, a)
        # the slot that is not found
        assert not r["metric"][w * MAX_REPORTS + 1].any() and not r["index"][w * MAX_REPORTS + 1].any()
        if variant == "b":
            silent = A.VARIANTS["b"]["silent"]
            assert float(rep["coarse_peak_array"][silent]) == 0.0 and silent not in xc
            assert sorted(xc) == [a for a in range(c[5]) if a != silent]
        else:
            assert sorted(xc) == list(range(c[5]))
    print(_id(p), "largest relative metric deviation from the restatement", worst)


def _check_combination(c, rep, got_m, got_i, n_lim=None):
    """the report against crosscorrelator.cpp:218-248 on the device's own table. The index: the device's x <= 1025
    (the largest xc_len) carries at most 8 products, 7 + 7 additions of the two sums and one division, 23 float32
    roundings of 2^-24 relative each, so it lies within 1025 * 23 * 2^-24 = 1.41e-3 < 2e-3 of the double value:
    further than 2e-3 from a half-integer the rounding is decided, inside that band either neighbour is accepted."""
    nt = A.sync_geometry(c)["n_templates"]
    ants = [a for a in range(n_lim or c[5]) if rep["coarse_peak_array"][a] > 0]
    ms, x, k_likely = A.combine(got_m, got_i, rep["coarse_peak_array"], nt, n_lim or c[5])
    for k in range(nt):
        s = np.float32(0)
        for a in ants:
            s = np.float32(s + got_m[a, k])
        assert abs(float(rep["fine_peak_metric"][k]) - float(s)) <= float(np.spacing(s)), (k, rep["fine_peak_metric"], s)
        ok = {int(np.floor(x[k] + 0.5))} if abs(x[k] - np.floor(x[k]) - 0.5) > 2e-3 else {int(np.floor(x[k])), int(np.ceil(x[k]))}
        assert int(rep["fine_peak_index"][k]) in ok, (k, x[k], rep["fine_peak_index"])
    assert not rep["fine_peak_metric"][nt:].any() and not rep["fine_peak_index"][nt:].any()
    assert int(rep["N_eff_TX"]) == 1 << k_likely
    assert int(rep["fine_peak_time_local"]) == int(rep["fine_peak_index"][k_likely])
    assert int(rep["fine_peak_time"]) == int(rep["coarse_peak_time"]) - A.sync_geometry(c)["xc_l"] + int(rep["fine_peak_time_local"])


@pytest.mark.parametrize("p", INPUTS, ids=_id)
def test_combination(p):
    c, variant = p
    r = _runs(p)
    n_eff = O.packet_sizes(O.psdef(*A.psdef(c)))["N_eff_TX"]
    for w in range(len(A.windows(c, variant))):
        rep = r["on"][w, 0]
        _check_combination(c, rep, r["metric"][w * MAX_REPORTS], r["index"][w * MAX_REPORTS])
        assert int(rep["N_eff_TX"]) == n_eff, (w, int(rep["N_eff_TX"]))


def test_the_feature_acts():
    c, nt = A.FOUR, A.sync_geometry(A.FOUR)["n_templates"]
    r = _runs((c, "c"))
    for w, (win, start, _, delays) in enumerate(A.windows(c, "c")):
        on, off = r["on"][w, 0], r["off"][w, 0]
        metric, index, _ = _restated(c, win, on)
        base = int(on["coarse_peak_time"]) - A.sync_geometry(c)["xc_l"]
        s = A.strongest(on["coarse_peak_array"], c[5])
        want_off = base + int(index[s, int(np.argmax(metric[s, :nt]))])
        _, x, k = A.combine(metric, index, on["coarse_peak_array"], nt)
        want_on = base + int(np.floor(x[k] + 0.5))
        assert int(off["fine_peak_time"]) == want_off == start + max(delays), (w, int(off["fine_peak_time"]), want_off)
        assert int(on["fine_peak_time"]) == want_on, (w, int(on["fine_peak_time"]), want_on, x[k])
        assert int(on["fine_peak_time"]) != int(off["fine_peak_time"])
    r = _runs((c, "a"))
    for w, (_, start, _, delays) in enumerate(A.windows(c, "a")):
        assert start + min(delays) <= int(r["on"][w, 0]["fine_peak_time"]) <= start + max(delays), w


def test_downstream_demodulation():
    import dnrp
    c = A.FOUR
    made = A.windows(c, "a")
    res = _runs((c, "a"))["on"]
    phy = _phy(c)
    ps = dnrp.psdef(*A.psdef(c))
    G = phy.packet_sizes(ps)["G"]
    iq = _to_dev(np.stack([m[0] for m in made]))
    pcc_llr = torch.zeros((len(made), 196), dtype=torch.int16, device="cuda:0")
    pdc_llr = torch.zeros((len(made), G), dtype=torch.int16, device="cuda:0")
    phy.rx_pcc_batch(dnrp.sync_reports(res[:, 0]), iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, m[2][2], m[2][3]) for i, m in enumerate(made)], iq, pdc_llr)
    phy.sync()
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    phy.close()
    for i, (_, _, meta, _) in enumerate(made):
        assert np.array_equal(g_pcc[i] > 0, np.unpackbits(meta[0])[:196] > 0), (i, "pcc bits")
        assert np.array_equal(g_pdc[i] > 0, np.unpackbits(meta[1])[:G] > 0), (i, "pdc bits")


def test_with_the_beta_search():
    cb = A.BETA_CASE  # a b = 1 packet in the stream of a b_max = 4 receiver, two antennas
    c = cb[:7]
    wins = [m[0] for m in K.windows(cb)]
    phy = _phy(c)
    phy.set_sync_beta_search(1)
    phy.set_sync_fine_all_antennas(1)
    res, cnt = _sync(phy, c, wins, chunk=K.chunk_len(cb))
    metric, index = phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
    phy.close()
    n_eff = O.packet_sizes(O.psdef(*K.psdef(cb)))["N_eff_TX"]
    for w, win in enumerate(wins):
        rep = res[w, 0]
        assert int(cnt[w]) == 1 and int(rep["b"]) == cb[7] and int(rep["N_eff_TX"]) == n_eff, (w, rep)
        _, want_i, xc = _restated(c, win, rep, b=cb[7])
        assert sorted(xc) == [0, 1]
        assert np.array_equal(index[w * MAX_REPORTS], want_i), (w, index[w * MAX_REPORTS], want_i)
        _check_combination(c, rep, metric[w * MAX_REPORTS], index[w * MAX_REPORTS])


def test_stream():
    import dnrp
    c = A.CASES[0]
    win, starts = A.two_packet_window(c)
    phy = _phy(c)
    phy.set_sync_fine_all_antennas(1)
    chunk, max_reports = 1024, 2
    sc = dnrp.SyncCfg(c[0], c[1], c[5], chunk, max_reports)
    S_win = phy.sync_stream_window(sc)
    n_chunks = -(-win.shape[1] // chunk)
    T = n_chunks * chunk + S_win
    rng = np.random.default_rng(79)
    sigma = np.sqrt(np.mean(np.abs(win[:, :starts[0] // 2]) ** 2) / 2)  # the window's own noise level
    stream = (sigma * (rng.standard_normal((c[5], T)) + 1j * rng.standard_normal((c[5], T)))).astype(np.complex64)
    stream[:, :win.shape[1]] = win
    g0 = 3 * T + T // 3  # the ring wraps inside the stream
    ring = np.zeros((c[5], T), np.complex64)
    ring[:, (g0 + np.arange(T)) % T] = stream
    res, chunk_of = phy.rx_sync_stream(sc, _to_dev(ring), g0, n_chunks, phy.sync_stream_init(sc))
    with pytest.raises(dnrp.DnrpError) as e:  # the table is not offered for the stream call
        phy.sync_fine_peaks(n_chunks * max_reports)
    assert e.value.code == -7
    phy.close()
    assert [int(r["fine_peak_time"]) - g0 for r in res] == starts
    nt, xc_l = A.sync_geometry(c)["n_templates"], A.sync_geometry(c)["xc_l"]
    for r, k in zip(res, chunk_of):
        t0 = g0 + int(k) * chunk
        cw = stream[:, int(k) * chunk: int(k) * chunk + S_win]
        metric, index, xc = A.antenna_peaks(cw, c, int(r["coarse_peak_time"]) - t0, float(r["cfo_fractional_rad"]),
                                            r["coarse_peak_array"])
        assert sorted(xc) == [0, 1]
        _, x, kl = A.combine(metric, index, r["coarse_peak_array"], nt)
        assert index[0, kl] == index[1, kl]  # no delay between the antennas: the mean is that index whatever the weights
        assert int(r["fine_peak_time"]) == int(r["coarse_peak_time"]) - xc_l + int(index[0, kl])
        assert int(r["N_eff_TX"]) == 1 << kl


def test_twice_the_same_bytes():
    p = (A.FOUR, "a")
    c, variant = p
    wins = [m[0] for m in A.windows(c, variant)]
    phy = _phy(c)
    phy.set_sync_fine_all_antennas(1)
    res, _ = _sync(phy, c, wins)
    metric, index = phy.sync_fine_peaks(len(wins) * MAX_REPORTS)
    phy.close()
    first = _runs(p)
    _same(res, first["on"])
    assert metric.tobytes() == first["metric"].tobytes() and index.tobytes() == first["index"].tobytes()
