"""GPU synchronisation parity on the geometry classes that the launchers of kernels/sync_*.hip choose by
size inside a template instantiation (tests/sync_grid_cases.py; tests/test_sync_grid_host.py proves the
inputs and the coverage): dnrp_rx_sync_batch against the oracle search on identical windows, with the
tolerances of tests/test_gpu_sync.py (_compare, unchanged): counts, detection, N_eff_TX and the fine
peak exact, the coarse peak within 1 DECT sample, the CFO within 2e-6 rad, metrics within 1e-3 relative.

 - every class in the [n][N_ant][S] layout, u2b12 in the per-antenna stream layout as well;
 - the classes with D / 8 > 512 run without split rounds whatever DNRP_SYNC_ROUNDS says (sync_peak_ok);
 - the step-sum switch forms at the new step sizes (wave kernel at step 48, single-prefetch stream
   kernel with 7 patterns, forced tranches at step 48);
 - the DNRP_EUNSUPPORTED exit of dnrp_rx_sync_batch, and the context after it;
 - GPU sync -> GPU PCC / PDC for a 7-pattern and a D / 8 > 512 class.

Measured on MI355X over all of the above (each test prints its own): coarse peak 0 samples off, CFO
3.7e-9 rad, detection metric 2.5e-7, coarse metric 6.6e-8, RMS 9.6e-8, fine metric 1.7e-7 relative.
A step walk that takes sq for a power of two (memory-safe, tried once) passes every older sync test and
fails here at step 48: parity of u2b12 and u1b12, the stream layout, the forced rounds and the tranches.
"""
import numpy as np
import pytest

import llr_gate
import oracle_py as O
import sync_grid_cases as G
from test_gpu_sync import _compare, _run
from test_gpu_sync_tranche import _check_equal

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -3


def _phy(ctx, lr=1, max_batch=4):
    import dnrp
    u_max, b_max, ntx, os_min, L, M = ctx
    phy = dnrp.Phy(u_max, b_max, ntx, os_min, L, M, chestim_mode_lr=bool(lr), max_batch=max_batch)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    return phy


def _sync(phy, case, stream_layout=False):
    import dnrp
    psd, ctx = G.case_def(case)
    sc = dnrp.SyncCfg(psd[0], psd[1], ctx[2], G.recipe(case)[1], G.MAX_REPORTS)
    return _run(phy, sc, G.windows(case)[0], G.MAX_REPORTS, stream_layout)


def _deviations(g, o):
    """largest deviation per toleranced field of one report (printed; the assertions are _compare's)"""
    nt = int(np.count_nonzero(o["xc_metric"]))
    na = int(np.count_nonzero(o["coarse_metric"]))
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) / np.asarray(b, np.float64) - 1)))
    return dict(coarse=abs(int(g["coarse_peak_time_local"]) - o["coarse_local"]),
                cfo=abs(float(g["cfo_fractional_rad"]) - o["cfo_frac"]),
                det_metric=rel(g["detection_metric"], o["det_metric"]),
                coarse_metric=rel(g["coarse_peak_array"][:na], o["coarse_metric"][:na]),
                rms=rel(g["rms_array"][:na], o["rms"][:na]),
                fine_metric=rel(g["fine_peak_metric"][:nt], o["xc_metric"][:nt]))


def _check(where, case, res, cnt):
    """the reports of the case's windows against the oracle's, the transmitted starts and the noise window"""
    refs, starts = G.oracle_reports(case), G.windows(case)[1]
    n_eff = O.packet_sizes(O.psdef(*G.case_def(case)[0]))["N_eff_TX"]
    worst = {}
    for w, ref in enumerate(refs):
        assert int(cnt[w]) == len(ref), (where, w, int(cnt[w]), len(ref))
        for k, o in enumerate(ref):
            for f, v in _deviations(res[w, k], o).items():
                worst[f] = max(worst.get(f, 0), v)
        for k, o in enumerate(ref):
            _compare(res[w, k], o, (where, w, k))
        for k in range(len(ref), G.MAX_REPORTS):
            assert int(res[w, k]["found"]) == 0, (where, w, k)
        if w < len(starts):
            assert int(cnt[w]) == 1, (where, w)
            assert int(res[w, 0]["fine_peak_time"]) == starts[w], (where, w, int(res[w, 0]["fine_peak_time"]), starts[w])
            assert int(res[w, 0]["N_eff_TX"]) == n_eff, (where, w)
    assert len(refs) == len(starts) + 1 and int(cnt[len(starts)]) == 0, where  # the noise window
    print("sync grid", where, "largest deviations", worst)


@pytest.mark.parametrize("name,stream_layout", [(n, False) for n in G.NAMES] + [("u2b12", True)],
                         ids=G.NAMES + ["u2b12-streams"])
def test_sync_grid_parity(name, stream_layout):
    phy = _phy(G.CASES[name][1], G.lr(name))
    res, cnt = _sync(phy, name, stream_layout)
    phy.close()
    _check(name, name, res, cnt)


@pytest.mark.parametrize("name,split", [("os2_u2b16_tm1", False), ("os2_C4", False), ("os2_u2b12", True),
                                        ("u1b2", True), ("u1b12", True), ("u1b16", True), ("lm1_u1b2", True),
                                        ("os2_u1b12", True)])
def test_forced_rounds(name, split, monkeypatch):
    """D / 8 > 512 (sync_peak_ok false): no split round is launched even when DNRP_SYNC_ROUNDS asks for two,
    so the inline detection alone is what the parity above compares; the os_min 2 class below that size
    does launch them. The 7-pattern classes have one antenna and so run without split rounds by default:
    with two rounds asked for, sync_peak_kernel<.., 6> and the split detection run at b > 1."""
    monkeypatch.setenv("DNRP_TIMING", "1")
    monkeypatch.setenv("DNRP_SYNC_ROUNDS", "2")
    phy = _phy(G.CASES[name][1], G.lr(name))
    phy.kernel_time_total("sync_peak", reset=True)
    phy.kernel_time_total("sync_detect", reset=True)
    res, cnt = _sync(phy, name)
    peaks = phy.kernel_time_total("sync_peak", reset=True)[1]
    detects = phy.kernel_time_total("sync_detect", reset=True)[1]
    phy.close()
    assert detects >= 1
    assert (peaks > 0) == split, (name, peaks)
    _check((name, "rounds 2"), name, res, cnt)


@pytest.mark.parametrize("name,env", [("u2b12", {"DNRP_SYNC_STREAM": "0"}),   # wave kernel at step 48
                                      ("u1b12", {"DNRP_SYNC_STREAM": "0"}),   # ... with 7 patterns
                                      ("u1b16", {"DNRP_SYNC_PIPE": "0"})])    # stream kernel <.., 16, 1>, 7 patterns
def test_switch_forms(name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    phy = _phy(G.CASES[name][1])
    res, cnt = _sync(phy, name)
    phy.close()
    _check((name, env), name, res, cnt)


def test_tranches_at_step_48(monkeypatch):
    """u2b12 (144 steps) with forced tranches 32,64 (frontiers 32, 96, 144): the oracle's reports, and every
    field equal to the one-tranche run by the rule of tests/test_gpu_sync_tranche.py"""
    name = "u2b12"
    assert G.sync_geometry(name)["step"] == 48
    phy = _phy(G.CASES[name][1])
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "0")
    res0, cnt0 = _sync(phy, name)
    monkeypatch.setenv("DNRP_SYNC_TRANCHE", "32,64")
    res, cnt = _sync(phy, name)
    phy.close()
    _check((name, "tranches 32,64"), name, res, cnt)
    _check_equal((name, "tranches 32,64"), res, cnt, res0, cnt0)


def test_sync_unsupported_geometry():
    """40/27, os_min 2, b 16, u 2 needs a 16384-point fine search (more than 160 KiB of LDS):
    DNRP_EUNSUPPORTED. The (2, 2) class of the same context then matches the oracle: the refused call
    left nothing queued."""
    import dnrp
    phy = _phy(G.UNSUPPORTED_CTX)
    case = G.UNSUPPORTED_FOLLOWUP
    wins = G.windows(case)[0]
    n_ant, S = wins[0].shape
    t = torch.from_numpy(np.stack(wins).view(np.float32).reshape(len(wins), n_ant, S, 2)).to("cuda:0")
    sc = dnrp.SyncCfg(*G.UNSUPPORTED_SYNC, 1, G.recipe(case)[1], G.MAX_REPORTS)
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_sync_batch(sc, t, len(wins), S, n_ant * S, S)
    assert e.value.code == EUNSUPPORTED
    phy.sync()
    res, cnt = _sync(phy, case)
    phy.close()
    _check("after the refusal", case, res, cnt)


@pytest.mark.parametrize("name", ["u1b12", "os2_C4"])
def test_sync_grid_then_demodulate(name):
    """GPU sync -> GPU RX on two windows of one packet against the oracle RX fed the same (GPU) report, as
    tests/test_gpu_sync.py::test_sync_then_demodulate: int16 LLRs through llr_gate.check, the oracle's own
    search at the same fine peak and CFO."""
    import dnrp
    rng = np.random.default_rng(25)
    psd, cfgt = G.CASES[name]
    n_ant = cfgt[2]
    phy = _phy(cfgt, G.lr(name))
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    S = sz["N_samples_packet_os_rs"]
    pre = sz["N_samples_STF"] * cfgt[3] * cfgt[4] // cfgt[5]  # one STF of lead-in at the hw rate
    S_win = S + pre + 32
    chunk = S_win * 7 // 8
    windows, metas = [], []
    for i in range(2):
        cfo = rng.uniform(-1.75, 1.75) * 2 * np.pi / sz["N_b_DFT_os"]
        win, meta = G.sync_window(rng, name, S_win, [pre + int(rng.integers(0, 32))], cfo)
        windows.append(win)
        metas.append(meta[0])
    res, cnt = _run(phy, dnrp.SyncCfg(psd[0], psd[1], n_ant, chunk, 1), windows, 1)
    assert list(cnt) == [1, 1]
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack(windows).view(np.float32).reshape(2, n_ant, S_win, 2)).to(dev)
    reps = dnrp.sync_reports(res[:, 0])
    pcc_llr = torch.zeros((2, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((2, sz["G"]), dtype=torch.int16, device=dev)
    phy.rx_pcc_batch(reps, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, m[2], m[3]) for i, m in enumerate(metas)], iq, pdc_llr)
    phy.sync()
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    phy.close()
    ocf = O.cfg(cfgt[0], cfgt[1], os_min=cfgt[3], L=cfgt[4], M=cfgt[5], lr=G.lr(name))
    osc = G.oracle_sync_cfg(name, chunk)
    for i, win in enumerate(windows):
        o = O.sync(osc, win, max_reports=1)[0]
        fine, cfo_g = int(res[i, 0]["fine_peak_time"]), float(res[i, 0]["cfo_fractional_rad"])
        assert o["fine_64"] == fine and abs(o["cfo_frac"] - cfo_g) < 2e-6, (name, i, o["fine_64"], fine)
        r = O.rx(ocf, O.psdef(*psd), win, fine, cfo_g, metas[i][2], metas[i][3])
        llr_gate.check((name, i, "pcc"), g_pcc[i], r["pcc_llr"])
        llr_gate.check((name, i, "pdc"), g_pdc[i], r["pdc_llr"])
        bits = np.unpackbits(metas[i][1])[: sz["G"]]
        assert np.mean((g_pdc[i] > 0).astype(np.uint8) != bits) < 2e-2, name
