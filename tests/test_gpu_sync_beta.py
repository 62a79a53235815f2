"""Beta search of the synchronisation on the GPU (dnrp_ctx_set_sync_beta_search; kernels/sync_fine.hip
sync_beta_kernel, sync_beta_decide, the per-b template rows of sync_fine_kernel): packets of every
b <= b_max in the stream of a b_max receiver, inputs of tests/sync_beta_cases.py (30 dB, MCS 1, random
mixing, CFO within +-1.75 subcarriers; tests/test_sync_beta_host.py proves their margin to the threshold).

1. L = M = 1, b_max / b an integer: every gate of tests/test_gpu_sync.py (same tolerances) against the
   oracle search of the class (u, b) at os_min b_max / b -- the same bos, geometry and template.
2. 10/9, 40/27 and b_max / b not an integer: the transmitted truth (b, N_eff_TX), then the chain GPU sync
   -> GPU PCC / PDC: every hard decision equals the transmitted d-bit and the LLRs pass the gate against
   the oracle RX fed the same report.
3. The ratio through the threshold: 1 dB below the numpy ratio of the last widening step the report says
   b, 1 dB above it the b below (float rounding moves the ratio by far less, a wrong band edge or
   normalisation by more).
4. Mixed b in one batch, in one window and in a ring searched by rx_sync_stream.
5. Off (the default) is the synchronisation as before: b = SyncCfg.b, byte-identical results.
"""
import numpy as np
import pytest

import llr_gate
import oracle_py as O
import sync_beta_cases as K

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _phy(c, max_batch=8):
    import dnrp
    u, b_max, os_min, L, M, n_ant, _, _ = c
    phy = dnrp.Phy(u, b_max, n_ant, os_min, L, M, max_batch=max_batch)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    return phy


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(*a.shape, 2)).to("cuda:0")


def _sync(phy, c, wins, max_reports=1, chunk=None):
    """rx_sync_batch of the windows (complex64 [n_ant, S] each) with the case's class as SyncCfg"""
    import dnrp
    n, (n_ant, S) = len(wins), wins[0].shape
    sc = dnrp.SyncCfg(c[0], c[1], n_ant, chunk or K.chunk_len(c), max_reports)
    res, cnt = phy.rx_sync_batch(sc, _to_dev(np.stack(wins)), n, S, n_ant * S, S)
    phy.sync()
    return res, cnt


def _compare(g, o, where):  # tests/test_gpu_sync.py::_compare, the same tolerances
    assert int(g["found"]) == o["found"] == 1, where
    assert int(g["detection_ant_idx"]) == o["det_ant"], where
    assert int(g["detection_time_local"]) == o["det_time"], (where, int(g["detection_time_local"]), o["det_time"])
    assert abs(int(g["coarse_peak_time_local"]) - o["coarse_local"]) <= 1, (where, int(g["coarse_peak_time_local"]),
                                                                            o["coarse_local"])
    assert int(g["N_eff_TX"]) == o["N_eff_TX"], where
    assert int(g["fine_peak_time"]) == o["fine_64"], (where, int(g["fine_peak_time"]), o["fine_64"])
    assert abs(float(g["cfo_fractional_rad"]) - o["cfo_frac"]) < 2e-6, (where, float(g["cfo_fractional_rad"]),
                                                                         o["cfo_frac"])
    np.testing.assert_allclose(g["detection_metric"], o["det_metric"], rtol=1e-3)
    np.testing.assert_allclose(g["coarse_peak_array"], o["coarse_metric"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(g["rms_array"], o["rms"], rtol=1e-3, atol=1e-7)
    nt = int(np.count_nonzero(o["xc_metric"]))
    np.testing.assert_allclose(g["fine_peak_metric"][:nt], o["xc_metric"][:nt], rtol=1e-3)


def test_setting_round_trip():
    phy = _phy(K.PARITY[0])
    assert phy.sync_beta_search()[:2] == (False, -10.0)  # the defaults
    for db in (-10.0, -3.0, 0.0):
        phy.set_sync_beta_search(1, db)
        on, got_db, lin = phy.sync_beta_search()
        assert on is True and got_db == np.float32(db)
        assert abs(lin - 10 ** (db / 20)) <= 2 * np.spacing(np.float32(10 ** (db / 20))), (db, lin)
    phy.set_sync_beta_search(1)
    assert phy.sync_beta_search()[:2] == (True, -10.0)
    import dnrp
    for bad in ((2, -10.0), (1, float("nan")), (1, float("inf")), (1, float("-inf"))):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_sync_beta_search(*bad)
        assert e.value.code == -1
    assert phy.sync_beta_search()[:2] == (True, -10.0)  # a refused call changes nothing
    phy.set_sync_beta_search(0)
    assert phy.sync_beta_search()[0] is False
    phy.close()


@pytest.mark.parametrize("c", K.PARITY, ids=K.case_id)
def test_parity_with_the_oracle_of_b(c):
    phy = _phy(c)
    phy.set_sync_beta_search(1)
    made = K.windows(c)
    res, cnt = _sync(phy, c, [m[0] for m in made])
    osc = K.oracle_sync_cfg(c)
    for w, (win, start, _, _) in enumerate(made):
        ref = O.sync(osc, win, max_reports=1)
        assert int(cnt[w]) == len(ref) == 1
        assert int(res[w, 0]["b"]) == c[7], (w, int(res[w, 0]["b"]))
        assert int(res[w, 0]["u"]) == c[0] and float(res[w, 0]["cfo_integer_rad"]) == 0.0
        _compare(res[w, 0], ref[0], (K.case_id(c), w))
        assert int(res[w, 0]["fine_peak_time"]) == start
    phy.close()


@pytest.mark.parametrize("c", K.TRUTH, ids=K.case_id)
def test_truth_then_demodulate(c):
    import dnrp
    u, b_max, os_min, L, M, n_ant, _, b = c
    phy = _phy(c)
    phy.set_sync_beta_search(1)
    made = K.windows(c)
    wins = [m[0] for m in made]
    res, cnt = _sync(phy, c, wins)
    ops = O.psdef(*K.psdef(c))
    sz = O.packet_sizes(ops)
    for w in range(len(made)):
        assert int(cnt[w]) == 1
        assert int(res[w, 0]["b"]) == b and int(res[w, 0]["N_eff_TX"]) == sz["N_eff_TX"], (w, res[w, 0])
    ps = dnrp.psdef(*K.psdef(c))
    G = phy.packet_sizes(ps)["G"]
    iq = _to_dev(np.stack(wins))
    reps = dnrp.sync_reports(res[:, 0])
    pcc_llr = torch.zeros((len(made), 196), dtype=torch.int16, device="cuda:0")
    pdc_llr = torch.zeros((len(made), G), dtype=torch.int16, device="cuda:0")
    phy.rx_pcc_batch(reps, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, m[2][2], m[2][3]) for i, m in enumerate(made)], iq, pdc_llr)
    phy.sync()
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    ocf = O.cfg(u, b_max, os_min=os_min, L=L, M=M)
    for i, (win, _, meta, _) in enumerate(made):
        assert np.array_equal(g_pcc[i] > 0, np.unpackbits(meta[0])[:196] > 0), (i, "pcc bits")
        assert np.array_equal(g_pdc[i] > 0, np.unpackbits(meta[1])[:G] > 0), (i, "pdc bits")
        r = O.rx(ocf, ops, win, int(res[i, 0]["fine_peak_time"]), float(res[i, 0]["cfo_fractional_rad"]), meta[2], meta[3])
        llr_gate.check((K.case_id(c), i, "pcc"), g_pcc[i], r["pcc_llr"])
        llr_gate.check((K.case_id(c), i, "pdc"), g_pdc[i], r["pdc_llr"])
    phy.close()


@pytest.mark.parametrize("c", [(1, 4, 1, 1, 1, 1, 0, 2), (1, 12, 1, 1, 1, 1, 0, 8)], ids=K.case_id)
def test_ratio_through_the_threshold(c):
    u, b_max, os_min, _, _, _, _, b = c
    phy = _phy(c)
    phy.set_sync_beta_search(1)
    win = K.windows(c)[0][0]
    res, _ = _sync(phy, c, [win])
    assert int(res[0, 0]["b"]) == b
    at = int(res[0, 0]["coarse_peak_time_local"])  # L = M = 1: a hw sample index of the window
    ratios = dict(K.band_ratios(win, u, b_max, os_min, at))
    r, below = ratios[b], K.B_IDX2B[K.B_IDX2B.index(b) - 1]
    # the steps before the last widening one must not stop the search at + 1 dB
    assert all(v > r * 10 ** (1.5 / 20) for bt, v in ratios.items() if bt < b), ratios
    for off_db, want in ((-1.0, b), (1.0, below)):
        phy.set_sync_beta_search(1, 20 * np.log10(r) + off_db)
        res, _ = _sync(phy, c, [win])
        assert int(res[0, 0]["found"]) == 1 and int(res[0, 0]["b"]) == want, (off_db, r, int(res[0, 0]["b"]))
    phy.close()


def _oracle_fine_of(c, win, chunk, k, max_reports=2):
    """the fine peak of the window's k-th packet by the oracle search of that packet's own b"""
    u, b_max, os_min, _, _, n_ant, _, b = c
    osc = O.sync_cfg(u, b, os_min=os_min * b_max // b, L=1, M=1, n_ant=n_ant, chunk_len=chunk)
    ref = O.sync(osc, win, max_reports=max_reports)
    assert len(ref) > k
    return ref[k]["fine_64"]


def test_mixed_b_in_one_batch():
    cs = [(1, 4, 1, 1, 1, 1, 0, b) for b in (1, 2, 4)]
    phy = _phy(cs[0])
    phy.set_sync_beta_search(1)
    made = [K.windows(c)[0] for c in cs]
    res, cnt = _sync(phy, cs[0], [m[0] for m in made])
    for w, (c, m) in enumerate(zip(cs, made)):
        assert int(cnt[w]) == 1 and int(res[w, 0]["b"]) == c[7]
        o = O.sync(K.oracle_sync_cfg(c), m[0], max_reports=1)[0]
        assert int(res[w, 0]["fine_peak_time"]) == o["fine_64"] == m[1]
    phy.close()


def test_two_b_in_one_window():
    ca, cb = K.MIXED_WINDOW
    phy = _phy(ca)
    phy.set_sync_beta_search(1)
    win, starts = K.two_packet_window(77, ca, cb)
    chunk = win.shape[1] - K.geometry(ca)["stf_hw"]
    res, cnt = _sync(phy, ca, [win], max_reports=2, chunk=chunk)
    assert int(cnt[0]) == 2
    for k, c in enumerate((ca, cb)):
        assert int(res[0, k]["b"]) == c[7], (k, int(res[0, k]["b"]))
        assert int(res[0, k]["fine_peak_time"]) == _oracle_fine_of(c, win, chunk, k) == starts[k]
    phy.close()


def test_two_b_in_a_ring():
    import dnrp
    ca, cb = K.MIXED_RING
    phy = _phy(ca)
    phy.set_sync_beta_search(1)
    win, starts = K.two_packet_window(78, ca, cb)
    chunk, max_reports = 2048, 2
    sc = dnrp.SyncCfg(1, 4, 1, chunk, max_reports)
    S_win = phy.sync_stream_window(sc)
    n_chunks = -(-win.shape[1] // chunk)
    T = n_chunks * chunk + S_win
    rng = np.random.default_rng(79)
    sigma = np.sqrt(np.mean(np.abs(win[:, :starts[0] // 2]) ** 2) / 2)  # the window's own noise level
    stream = (sigma * (rng.standard_normal((1, T)) + 1j * rng.standard_normal((1, T)))).astype(np.complex64)
    stream[:, :win.shape[1]] = win
    g0 = 3 * T + T // 3  # the ring wraps inside the stream
    ring = np.zeros((1, T), np.complex64)
    ring[:, (g0 + np.arange(T)) % T] = stream
    state = phy.sync_stream_init(sc)
    res, chunk_of = phy.rx_sync_stream(sc, _to_dev(ring), g0, n_chunks, state)
    assert [int(r["fine_peak_time"]) - g0 for r in res] == starts
    assert [int(r["b"]) for r in res] == [ca[7], cb[7]]
    for r, c, k in zip(res, (ca, cb), chunk_of):
        tk = int(k) * chunk
        cw = stream[:, tk:tk + S_win]
        u, b_max, os_min, _, _, n_ant, _, b = c
        ref = O.sync(O.sync_cfg(u, b, os_min=os_min * b_max // b, L=1, M=1, n_ant=n_ant, chunk_len=chunk), cw,
                     max_reports=max_reports)
        assert int(r["fine_peak_time"]) - g0 - tk in [o["fine_64"] for o in ref]
    phy.close()


def test_off_reports_the_class_b():
    c = (1, 4, 1, 1, 1, 1, 0, 1)
    phy = _phy(c)
    assert phy.sync_beta_search()[0] is False  # the default
    res, cnt = _sync(phy, c, [K.windows(c)[0][0]])
    assert int(cnt[0]) == 1 and int(res[0, 0]["b"]) == 4
    phy.close()


@pytest.mark.parametrize("c", [(1, 4, 1, 1, 1, 1, 0, 4), (2, 8, 1, 1, 1, 4, 5, 8), (1, 12, 1, 1, 1, 1, 0, 12)],
                         ids=K.case_id)
def test_on_equals_off_for_b_max_packets(c):
    phy = _phy(c)
    wins = [m[0] for m in K.windows(c)]
    off, cnt_off = _sync(phy, c, wins)
    phy.set_sync_beta_search(1)
    on, cnt_on = _sync(phy, c, wins)
    phy.set_sync_beta_search(0)
    off2, _ = _sync(phy, c, wins)
    assert list(cnt_off) == list(cnt_on) == [1] * len(wins)
    assert int(on[0, 0]["b"]) == c[7]
    assert on.tobytes() == off.tobytes() == off2.tobytes()
    phy.close()
