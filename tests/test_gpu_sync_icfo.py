"""Integer CFO search of the synchronisation on the GPU (dnrp_ctx_set_sync_icfo_search; kernels/sync_fine.hip
sync_icfo_kernel, sync_icfo_decide in sync_fine_kernel / sync_fine_ant_kernel / sync_fine_combine_kernel): packets
with a carrier offset of (4 k + f) subcarriers, inputs and the numpy restatement of tests/sync_icfo_cases.py
(tests/test_sync_icfo_host.py proves their margin).

1. Scores: the device table within 1e-3 of the row's largest entry of the restatement evaluated at the device
   report's own coarse peak and fractional CFO (the gate tests/test_gpu_sync_fine_ant.py uses for float transform
   metrics against numpy); the -1 columns exact. Not at 10/9: the tests have no numpy resampler.
2. Decision: k is the injected k on every window, cfo_integer_rad == float32(-k 8 pi / N) exactly.
3. Reports: at L = M = 1 every other field against the oracle search of the window with 4 k subcarriers taken out,
   the gates of tests/test_gpu_sync_beta.py::test_parity_with_the_oracle_of_b (fine peak and N_eff_TX exact). At
   10/9 the fine peak (exactly the hw sample the packet starts at) and N_eff_TX against the transmitted truth, then
   the chain GPU sync -> GPU PCC / PDC: every hard decision is
   the transmitted bit. Without the search these windows give another fine peak or N_eff_TX
   (test_off_misses_these_windows).
4. Demodulate: the reports of the first two cases at k = +-1 through rx_pcc_batch, every PCC LLR sign right.
5. Off: range 0 after having been on gives the bytes of a fresh context and no sync_icfo launch; a range on k = 0
   windows changes no report byte (cfo_integer_rad is +0).
6. Stream: a ring holding a k = +1 packet through rx_sync_stream gives the k and fine peak of the batch call.
7. Setter / getter round trip and the error codes.

With the beta search on as well, the candidates' cells are those of the first beta decision (the uncorrected
spectrum: for the b = 1 packet in b_max 8 at k = -4, f = -1.28 that is b = 2, ratio 0.399 against 0.316, and the
search still finds k = -4 through the hole at DC), so the restatement of item 1 takes sync_beta_cases.estimate_beta
at the device's coarse peak for b; the reported b is the second decision, on the spectrum moved back by 4 k bins,
and item 3 holds it to the oracle's.
"""
import numpy as np
import pytest

import oracle_py as O
import sync_beta_cases as K
import sync_icfo_cases as I

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -7, -1
L1 = [q for q in I.CASES if q.c[3] == q.c[4] == 1]


def _phy(q, max_batch=16):
    import dnrp
    u, b_max, os_min, L, M, n_ant, _, _ = q.c
    phy = dnrp.Phy(u, b_max, n_ant, os_min, L, M, max_batch=max_batch)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    if q.beta:
        phy.set_sync_beta_search(1)
    if q.fine_all:
        phy.set_sync_fine_all_antennas(1)
    return phy


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(*a.shape, 2)).to("cuda:0")


def _sync(phy, q, wins, chunk=None):
    import dnrp
    n, (n_ant, S) = len(wins), wins[0].shape
    sc = dnrp.SyncCfg(q.c[0], q.c[1], n_ant, chunk or K.chunk_len(q.c), 1)
    res, cnt = phy.rx_sync_batch(sc, _to_dev(np.stack(wins)), n, S, n_ant * S, S)
    phy.sync()
    return res, cnt


_RUNS = {}


def _run(q):
    """one searching call per case, shared by the tests: (reports [n], found counts, scores, k)"""
    if q.id not in _RUNS:
        phy = _phy(q)
        phy.set_sync_icfo_search(q.rng)
        wins = [w[1] for w in I.all_windows(q)]
        res, cnt = _sync(phy, q, wins)
        score, k = phy.sync_icfo_scores(len(wins))
        phy.close()
        _RUNS[q.id] = (res[:, 0].copy(), cnt.copy(), score, k)
    return _RUNS[q.id]


def test_setting_round_trip_and_errors():
    import dnrp
    q = I.BASE
    phy = _phy(q)
    assert phy.sync_icfo_search() == 0  # the default
    for r in (1, 4, 2):
        phy.set_sync_icfo_search(r)
        assert phy.sync_icfo_search() == r
    with pytest.raises(dnrp.DnrpError) as e:
        phy.set_sync_icfo_search(5)
    assert e.value.code == EINVAL and phy.sync_icfo_search() == 2  # a refused call changes nothing
    with pytest.raises(dnrp.DnrpError) as e:  # no searching call yet
        phy.sync_icfo_scores(1)
    assert e.value.code == ESTATE
    wins = [w[0] for w in I.windows(q, 1)]
    _sync(phy, q, wins)
    with pytest.raises(dnrp.DnrpError) as e:
        phy.sync_icfo_scores(len(wins) + 1)
    assert e.value.code == EINVAL
    score, k = phy.sync_icfo_scores(len(wins))
    assert score.shape == (len(wins), 8, 9) and list(k) == [1] * len(wins)
    phy.set_sync_icfo_search(0)
    _sync(phy, q, wins)
    with pytest.raises(dnrp.DnrpError) as e:  # the latest call ran off
        phy.sync_icfo_scores(len(wins))
    assert e.value.code == ESTATE
    phy.close()


@pytest.mark.parametrize("q", L1, ids=lambda q: q.id)
def test_scores_against_numpy(q):
    u, _, _, _, _, n_ant, _, _ = q.c
    res, cnt, score, _ = _run(q)
    worst = 0.0
    for w, (k, win, _, _) in enumerate(I.all_windows(q)):
        assert int(cnt[w]) == 1 and int(res[w]["found"]) == 1
        at = int(res[w]["coarse_peak_time_local"])
        # the class b, or with the beta search on its first decision, on the uncorrected spectrum
        b = K.estimate_beta(win, u, q.c[1], q.c[2], at, 10 ** (-10 / 20))[0] if q.beta else q.c[1]
        ref = I.scores(win, u, q.N, b, at, float(res[w]["cfo_fractional_rad"]), q.rng)
        assert np.array_equal(score[w, :n_ant] == -1, ref == -1), (w, score[w, :n_ant], ref)
        assert np.all(score[w, n_ant:] == -1)
        for a in range(n_ant):
            live = ref[a] >= 0
            d = np.abs(score[w, a][live] - ref[a][live]).max() / ref[a].max()
            worst = max(worst, d)
            assert d <= 1e-3, (w, a, d, score[w, a], ref[a])
    print(q.id, "largest score difference / row maximum", worst)


@pytest.mark.parametrize("q", I.CASES, ids=lambda q: q.id)
def test_decision(q):
    res, cnt, score, k_dev = _run(q)
    for w, (k, _, _, _) in enumerate(I.all_windows(q)):
        assert int(cnt[w]) == 1, w
        assert int(k_dev[w]) == k, (w, k, int(k_dev[w]), score[w, :q.c[5]].sum(0))
        got = np.float32(res[w]["cfo_integer_rad"])
        assert got == I.rad_of(k, q.N) and not (k == 0 and np.signbit(got)), (w, k, got)
        assert I.decide(score[w, :q.c[5]])[0] == k  # the read-back k is the decision on the read-back table


def _compare(g, o, where, all_ant):  # tests/test_gpu_sync_beta.py::_compare, the same tolerances
    assert int(g["found"]) == o["found"] == 1, where
    assert int(g["detection_ant_idx"]) == o["det_ant"], where
    assert int(g["detection_time_local"]) == o["det_time"], (where, int(g["detection_time_local"]), o["det_time"])
    assert abs(int(g["coarse_peak_time_local"]) - o["coarse_local"]) <= 1, (where, int(g["coarse_peak_time_local"]),
                                                                            o["coarse_local"])
    assert int(g["N_eff_TX"]) == o["N_eff_TX"], (where, int(g["N_eff_TX"]), o["N_eff_TX"])
    assert int(g["fine_peak_time"]) == o["fine_64"], (where, int(g["fine_peak_time"]), o["fine_64"])
    assert abs(float(g["cfo_fractional_rad"]) - o["cfo_frac"]) < 2e-6, (where, float(g["cfo_fractional_rad"]),
                                                                         o["cfo_frac"])
    np.testing.assert_allclose(g["detection_metric"], o["det_metric"], rtol=1e-3)
    np.testing.assert_allclose(g["coarse_peak_array"], o["coarse_metric"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(g["rms_array"], o["rms"], rtol=1e-3, atol=1e-7)
    if not all_ant:  # the oracle correlates the strongest antenna only: its metrics are not the antenna sums
        nt = int(np.count_nonzero(o["xc_metric"]))
        np.testing.assert_allclose(g["fine_peak_metric"][:nt], o["xc_metric"][:nt], rtol=1e-3)


@pytest.mark.parametrize("q,k", [(q, k) for q in L1 for k in q.ks], ids=lambda v: v.id if isinstance(v, I.Case) else "k%d" % v)
def test_reports_equal_the_oracle_on_the_derotated_window(q, k):
    res, _, _, _ = _run(q)
    osc = K.oracle_sync_cfg(q.c)
    n_eff = O.packet_sizes(O.psdef(*K.psdef(q.c)))["N_eff_TX"]
    for w, (kw, win, start, _) in enumerate(I.all_windows(q)):
        if kw != k:
            continue
        ref = O.sync(osc, I.derotate(win, k, q.N), max_reports=1)
        assert len(ref) == 1 and ref[0]["fine_64"] == start and ref[0]["N_eff_TX"] == n_eff  # the oracle is exact there
        assert int(res[w]["b"]) == q.c[7] and int(res[w]["u"]) == q.c[0], (w, int(res[w]["b"]))
        _compare(res[w], ref[0], (q.id, k, w), q.fine_all)


def test_off_misses_these_windows():
    """what the search is for: with the setting off every k != 0 window of the base cases is found, with the
    right fractional CFO, and with another fine peak or N_eff_TX than the transmitted one"""
    for q in (I.BASE, I.TWO_TX):
        n_eff = O.packet_sizes(O.psdef(*K.psdef(q.c)))["N_eff_TX"]
        made = [m for m in I.all_windows(q) if m[0] != 0]
        phy = _phy(q)
        res, cnt = _sync(phy, q, [m[1] for m in made])
        phy.close()
        for w, (k, _, start, _) in enumerate(made):
            assert int(cnt[w]) == 1 and float(res[w, 0]["cfo_integer_rad"]) == 0.0
            assert int(res[w, 0]["fine_peak_time"]) != start or int(res[w, 0]["N_eff_TX"]) != n_eff, (q.id, k, w)


def _demodulate(q, made, res, pdc):
    """GPU PCC (and PDC) of the windows with the device reports: every hard decision is the transmitted bit"""
    import dnrp
    phy = _phy(q)
    ps = dnrp.psdef(*K.psdef(q.c))
    G = phy.packet_sizes(ps)["G"]
    iq = _to_dev(np.stack([m[1] for m in made]))
    pcc_llr = torch.zeros((len(made), 196), dtype=torch.int16, device="cuda:0")
    pdc_llr = torch.zeros((len(made), G), dtype=torch.int16, device="cuda:0")
    phy.rx_pcc_batch(dnrp.sync_reports(res), iq, pcc_llr)
    if pdc:
        phy.rx_pdc_batch([dnrp.PdcReq(ps, i, m[3][2], m[3][3]) for i, m in enumerate(made)], iq, pdc_llr)
    phy.sync()
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    phy.close()
    for i, m in enumerate(made):
        assert np.array_equal(g_pcc[i] > 0, np.unpackbits(m[3][0])[:196] > 0), (q.id, m[0], i, "pcc bits")
        if pdc:
            assert np.array_equal(g_pdc[i] > 0, np.unpackbits(m[3][1])[:G] > 0), (q.id, m[0], i, "pdc bits")


def test_resampled_truth_then_demodulate():
    q = I.RESAMPLED
    res, cnt, _, _ = _run(q)
    made = I.all_windows(q)
    n_eff = O.packet_sizes(O.psdef(*K.psdef(q.c)))["N_eff_TX"]
    for w in range(len(made)):
        assert int(cnt[w]) == 1
        assert int(res[w]["b"]) == q.c[7] and int(res[w]["N_eff_TX"]) == n_eff, (w, made[w][0], res[w])
        # the fine peak: exactly the hw sample the packet was put at. The templates are the transmitter's own
        # chain (STF through the TX resampler, its delay included), so the correlation peaks at the packet's first
        # sample; it is the gate bench.py counts its fine-peak errors with on 10/9 windows (fine_peak_time != offset)
        print(q.id, "k", made[w][0], "fine peak - start", int(res[w]["fine_peak_time"]) - made[w][2])
        assert int(res[w]["fine_peak_time"]) == made[w][2], (w, made[w][0], int(res[w]["fine_peak_time"]), made[w][2])
    _demodulate(q, made, res, pdc=True)


@pytest.mark.parametrize("q", [I.BASE, I.TWO_TX], ids=lambda q: q.id)
def test_pcc_with_the_reports(q):
    res, _, _, _ = _run(q)
    pick = [w for w, m in enumerate(I.all_windows(q)) if abs(m[0]) == 1]
    _demodulate(q, [I.all_windows(q)[w] for w in pick], res[pick], pdc=False)


def test_off_is_the_synchronisation_as_it_is(monkeypatch):
    monkeypatch.setenv("DNRP_TIMING", "1")
    q = I.TWO_TX
    made = I.all_windows(q)
    wins = [m[1] for m in made]
    zero = [w for w, m in enumerate(made) if m[0] == 0]
    fresh = _phy(q)
    off, cnt_off = _sync(fresh, q, wins)
    assert fresh.kernel_time_total("sync_icfo")[1] == 0
    fresh.close()
    phy = _phy(q)
    phy.set_sync_icfo_search(q.rng)
    on, cnt_on = _sync(phy, q, wins)
    assert phy.kernel_time_total("sync_icfo")[1] == 1
    phy.set_sync_icfo_search(0)
    off2, cnt_off2 = _sync(phy, q, wins)
    assert phy.kernel_time_total("sync_icfo")[1] == 0
    phy.close()
    assert list(cnt_off) == list(cnt_on) == list(cnt_off2) == [1] * len(wins)
    assert off2.tobytes() == off.tobytes()
    assert np.all(off["cfo_integer_rad"] == 0) and not np.any(np.signbit(off["cfo_integer_rad"]))
    # a range on k = 0 windows: the decision is 0, written as +0, and nothing else moves
    assert len(zero) == I.N_WINDOWS and on[zero].tobytes() == off[zero].tobytes()
    assert on.tobytes() != off.tobytes()  # the k != 0 windows do move


def test_stream_equals_batch():
    import dnrp
    q = I.BASE
    k, win, start, _ = [m for m in I.all_windows(q) if m[0] == 1][0]
    n_ant = q.c[5]
    res_b, _, _, _ = _run(q)
    w = [i for i, m in enumerate(I.all_windows(q)) if m[0] == 1][0]
    assert int(res_b[w]["fine_peak_time"]) == start
    phy = _phy(q)
    phy.set_sync_icfo_search(q.rng)
    chunk = 1024
    sc = dnrp.SyncCfg(q.c[0], q.c[1], n_ant, chunk, 1)
    S_win = phy.sync_stream_window(sc)
    n_chunks = -(-win.shape[1] // chunk)
    T = n_chunks * chunk + S_win
    rng = np.random.default_rng(81)
    sigma = np.sqrt(np.mean(np.abs(win[:, :start // 2]) ** 2) / 2)  # the window's own noise level
    stream = (sigma * (rng.standard_normal((n_ant, T)) + 1j * rng.standard_normal((n_ant, T)))).astype(np.complex64)
    stream[:, :win.shape[1]] = win
    g0 = 3 * T + T // 3  # the ring wraps inside the stream
    ring = np.zeros((n_ant, T), np.complex64)
    ring[:, (g0 + np.arange(T)) % T] = stream
    res, _ = phy.rx_sync_stream(sc, _to_dev(ring), g0, n_chunks, phy.sync_stream_init(sc))
    with pytest.raises(dnrp.DnrpError) as e:  # the table is not offered for the stream call
        phy.sync_icfo_scores(n_chunks)
    assert e.value.code == ESTATE
    phy.close()
    assert [int(r["fine_peak_time"]) - g0 for r in res] == [start]
    assert np.float32(res[0]["cfo_integer_rad"]) == np.float32(res_b[w]["cfo_integer_rad"]) == I.rad_of(1, q.N)
    assert int(res[0]["N_eff_TX"]) == int(res_b[w]["N_eff_TX"])
