"""GPU RX parity on frequency-selective, time-varying channels with a timing error in the sync report
(tests/rx_selective_cases.py; tests/test_rx_selective_host.py proves on the CPU that these windows are fair
for a float32 receiver, that they carry |STO| >= 0.5 samples, |H| varying over the band and taps drifting over
the packet, and that a receiver with the STO ramp's sign wrong, the Wiener weights reversed or the left DRS
symbol held fails the gate on them).

Every other RX parity table runs over one flat, constant matrix per packet (1 + 0j for SISO) with the packet
start known to the sample, so the derotation ramp is about zero and every pilot window sees the same value.
Here the same oracle and the same gates (_check_rx unchanged: llr_gate on PCC and PDC, SNR reports within
0.05 dB, STO within 1e-3 samples, RMS within 1e-4 relative, MIMO report exact) meet

 - every row of rx_selective_cases.RUNS on the receiver it is named for, proved by launch counts
   (DNRP_TIMING=1): epoch, fused, the Y path's cells kernel, the MMSE cells kernel, and the default path of
   the other front ends and resamplers;
 - the epoch receiver against the Y path on the same windows;
 - GPU sync -> GPU RX on two windows through the same channel, where the multipath alone sets the timing.

The uncoded error rates of these windows are bounded on the CPU (the oracle's, test_rx_selective_host.py),
not here: 256-QAM over such a channel is well above _rx_parity's 2 % bound for flat channels.
"""
import numpy as np
import pytest

import llr_gate
import oracle_py as O
import rx_grid_cases as G
import rx_selective_cases as S
from test_gpu_parity import _check_rx, _gpu_rx, _rx_parity

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_ENV = ("DNRP_RX_EPOCH", "DNRP_RX_FUSED", "DNRP_RX_SNR_FRONT", "DNRP_RX_GROUP")


def _env(monkeypatch, name, receiver):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    if receiver not in ("default", "sm"):
        for k, v in G.env_of(name, receiver).items():
            monkeypatch.setenv(k, v)
    monkeypatch.setenv("DNRP_TIMING", "1")


def _phy(name, lr, stride):
    import dnrp
    u_max, b_max, n_rx, os_min, L, M = S.spec(name)[1]
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, chestim_mode_lr=bool(lr), stride=stride, max_batch=4)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    return phy


def _reports(name):
    import dnrp
    psd = S.spec(name)[0]
    n_eff = O.packet_sizes(O.psdef(*psd))["N_eff_TX"]
    reports = []
    for w in S.windows(name):
        rep = dnrp.SyncReport(w["fine_peak"], w["cfo_est"], 0.0, psd[0], psd[1], n_eff)
        assert float(np.float32(rep.cfo_fractional_rad)) == w["cfo_est"]
        if w["sync_rms"] is not None:
            rep.rms[0] = w["sync_rms"][0]
        reports.append(rep)
    return reports


def _prepared(name, lr, stride):
    """the case's windows in the form _rx_parity takes, with a context of its own; no hard-decision bound
    (module docstring)"""
    import dnrp
    psd = S.spec(name)[0]
    ws = S.windows(name)
    return (_phy(name, lr, stride), dnrp.psdef(*psd), O.psdef(*psd), [w["win"] for w in ws], _reports(name),
            [w["nid"] for w in ws], [w["pt"] for w in ws], [w["pdc"] for w in ws], [False] * len(ws),
            lambda i: S.oracle(name, i, lr, stride))


def _counts(phy):
    return {k: phy.kernel_time_total(k)[1] for k in ("rx_epoch", "rx_fused", "rx_pdc", "rx_fft_pcc", "rx_pdc_phase")}


def _sm_parity(name, lr, stride):
    """spatial multiplexing through the MMSE receiver, the checks of test_gpu_parity._rx_sm_parity: _check_rx with
    the PCC report, the PDC SNR report within 0.05 dB"""
    import dnrp
    psd = S.spec(name)[0]
    ws = S.windows(name)
    phy = _phy(name, lr, stride)
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    assert sz["N_SS"] > 1
    phy.set_rx_mode(phy.RX_MODE_SM_MMSE)
    g_pcc, g_pdc, rep1, rep2 = _gpu_rx(phy, ps, sz, [w["win"] for w in ws], _reports(name), [w["nid"] for w in ws],
                                       [w["pt"] for w in ws])
    for i in range(len(ws)):
        r = S.oracle(name, i, lr, stride)
        _check_rx((name, "sm", i), g_pcc[i], g_pdc[i], rep1[i], None, r)
        assert abs(rep2[i].snr_dB - r["snr_pdc"]) < 0.05, (name, i, rep2[i].snr_dB, r["snr_pdc"])
    return phy


@pytest.mark.parametrize("name,receiver,lr,stride", S.RUNS,
                         ids=[f"{n}-{r}-{'lr' if lr else 'l'}-s{st}" for n, r, lr, st in S.RUNS])
def test_rx_selective_parity(name, receiver, lr, stride, monkeypatch):
    import dnrp
    _env(monkeypatch, name, receiver)
    psd, ctx = S.spec(name)[:2]
    wave = G.wave_geometry(psd, ctx)
    if receiver == "fused":
        assert int(dnrp.query_table("fused_lds_bytes", ctx[2])[0]) <= 160 * 1024
    if receiver == "sm":
        phy = _sm_parity(name, lr, stride)
    else:
        phy = _rx_parity((name, receiver, lr, stride), stride, _prepared(name, lr, stride))
    c = _counts(phy)
    phy.close()
    # the run is on the receiver it is named for: no case passes on a fallback
    if receiver == "epoch":
        assert wave and c["rx_epoch"] > 0 and c["rx_fused"] == 0, (name, c)
    elif receiver == "fused":
        assert wave and c["rx_fused"] > 0 and c["rx_epoch"] == 0, (name, c)
    else:  # the Y path and the cells kernel ("default": no case of that list is a 4-antenna wave geometry)
        assert receiver != "default" or not (wave and ctx[2] >= 4), name
        assert c["rx_epoch"] == 0 and c["rx_fused"] == 0 and c["rx_pdc"] > 0, (name, c)
    assert c["rx_fft_pcc"] > 0 and c["rx_pdc_phase"] == 0, (name, c)


@pytest.mark.parametrize("name", ["r22_256", "r11_256"])
def test_epoch_agrees_with_ypath(name, monkeypatch):
    """the epoch receiver's LLRs against the Y path's on the same windows, through the gate"""
    import dnrp
    psd = S.spec(name)[0]
    ws = S.windows(name)
    out = {}
    for receiver in ("epoch", "ypath"):
        _env(monkeypatch, name, receiver)
        phy = _phy(name, 1, 2)
        ps = dnrp.psdef(*psd)
        out[receiver] = _gpu_rx(phy, ps, phy.packet_sizes(ps), [w["win"] for w in ws], _reports(name),
                                [w["nid"] for w in ws], [w["pt"] for w in ws])
        c = _counts(phy)
        phy.close()
        assert (c["rx_epoch"] > 0) == (receiver == "epoch") and c["rx_fused"] == 0, (name, receiver, c)
    for i in range(len(ws)):
        llr_gate.check((name, i, "pcc", "epoch against ypath"), out["epoch"][0][i], out["ypath"][0][i])
        llr_gate.check((name, i, "pdc", "epoch against ypath"), out["epoch"][1][i], out["ypath"][1][i])
        assert out["epoch"][3][i].snr_dB == pytest.approx(out["ypath"][3][i].snr_dB, abs=0.05)


@pytest.mark.parametrize("name", sorted(S.SYNC_CASES))
def test_sync_then_demodulate_selective(name, monkeypatch):
    """GPU sync on a window through the selective channel against the oracle's search (test_gpu_sync._compare:
    fine peak and N_eff_TX exact), then the GPU's own report into the GPU RX and into the oracle RX."""
    import dnrp
    from test_gpu_sync import _compare, _run
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    w = S.sync_window(name)
    psd, (u_max, b_max, n_rx, os_min, L, M), lr = w["psd"], w["ctx"], w["lr"]
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, chestim_mode_lr=bool(lr), max_batch=4)
    phy.add_network_id(w["nid"])
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    S_win = w["win"].shape[1]
    res, cnt = _run(phy, dnrp.SyncCfg(psd[0], psd[1], n_rx, w["chunk"], 1), [w["win"]], 1)
    assert list(cnt) == [1]
    o = O.sync(w["osc"], w["win"], max_reports=1)[0]
    _compare(res[0, 0], o, (name, "selective"))
    assert int(res[0, 0]["N_eff_TX"]) == sz["N_eff_TX"]
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(w["win"].view(np.float32).reshape(1, n_rx, S_win, 2).copy()).to(dev)
    pcc_llr = torch.zeros((1, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((1, sz["G"]), dtype=torch.int16, device=dev)
    rep1 = phy.rx_pcc_batch(dnrp.sync_reports(res[:, 0]), iq, pcc_llr, want_report=True)
    rep2 = phy.rx_pdc_batch([dnrp.PdcReq(ps, 0, w["nid"], w["pt"])], iq, pdc_llr, want_report=True)
    phy.sync()
    fine, cfo_g = int(res[0, 0]["fine_peak_time"]), float(res[0, 0]["cfo_fractional_rad"])
    r = O.rx(w["ocf"], w["ops"], w["win"], fine, cfo_g, w["nid"], w["pt"])
    assert abs(r["sto"]) >= 1.5, (name, r["sto"])  # the timing error the multipath leaves
    # the sync report's RMS values are kept by the receiver (rx_synced.cpp:620-655): not compared with the
    # oracle's own estimates
    llr_gate.check((name, "sync", "pcc"), pcc_llr[0].cpu().numpy(), r["pcc_llr"])
    llr_gate.check((name, "sync", "pdc"), pdc_llr[0].cpu().numpy(), r["pdc_llr"])
    assert abs(rep1[0].snr_dB - r["snr_pcc"]) < 0.05 and abs(rep1[0].sto_fractional - r["sto"]) < 1e-3, name
    assert abs(rep2[0].snr_dB - r["snr_pdc"]) < 0.05, name
    bits = np.unpackbits(w["pdc"])[: sz["G"]]
    assert np.mean((pdc_llr[0].cpu().numpy() > 0).astype(np.uint8) != bits) < 2e-2, name
    phy.close()
