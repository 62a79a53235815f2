"""GPU parity at the smallest shapes that reach the one-wavefront FFT's exchange addressing (wfft_ex,
device_common.hpp) and the front end's padded mixer stores (RX_MIX_PAD, wfft_index.hpp / rx_front.hpp).

mu = 1, beta = 16 (N_b_DFT_os = 1024), one slot (two with four transmit streams, which have no one-slot
packet at mu = 1), three packets per case: three packets make a grid that is no multiple of 8, so the
XCD-aware kernels run padding workgroups.
  * TX against the oracle for transmit diversity on 4 and 2 antennas (the one-hot bin forms TXS_TXDIV1)
    and SISO: relative L2 error per packet and antenna <= 1e-4, the gate of tests/test_gpu_parity.py.
  * RX through the epoch receiver (DNRP_RX_EPOCH=2) at (N_RX, N_eff_TX) = (4, 4), (4, 2), (2, 1), with twin
    units (DNRP_EQ_TWIN=1) and without, every packet under tests/llr_gate.py.
  * the Y path (rx_fft_wave_ct_kernel and the cell kernels) at (1, 1).
  * the second packet of every case starts three samples before its window (fine_peak < 0).
  * one case at MCS 1 (QPSK): the run-time N_bps instantiation, NBPS = 0.
The windows and the oracle's results are built once per case and shared.
"""
import functools

import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N_PKT = 3
# id: (tm_mode, mcs, N_RX, SNR dB)
CASES = {
    "rx4_tx4": (5, 8, 4, 30.0),
    "rx4_tx2": (1, 8, 4, 30.0),
    "rx2_tx1": (0, 8, 2, 30.0),
    "rx1_tx1": (0, 8, 1, 30.0),
    "rx4_tx4_qpsk": (5, 1, 4, 12.0),
}
PEAKS = (7, -3, 0)  # packet 1 starts before its window


def _psd(name):
    tm, mcs, _, _ = CASES[name]
    return (1, 16, 1, 2 if tm == 5 else 1, tm, mcs)  # four transmit streams: no one-slot packet at mu = 1


@functools.lru_cache(maxsize=None)
def _inputs(name):
    tm, mcs, n_rx, snr = CASES[name]
    ocf, ops = O.cfg(1, 16, 1, 10, 9), O.psdef(*_psd(name))
    sz, dm = O.packet_sizes(ops), O.dims(ocf, ops)
    assert dm["N_b_DFT_os"] == 1024
    S = dm["N_packet_os_rs"]
    rng = np.random.default_rng(0xD1E7)
    out = []
    for i in range(N_PKT):
        pcc, pdc = O.pack_bits(F.random_bits(rng, 196)), O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt, fp = 100 + i, 1 + i % 2, PEAKS[i]
        x, _ = O.tx(ocf, ops, pcc, pdc, S, network_id=nid, plcf_type=pt)
        cfo = rng.uniform(-1.0, 1.0) * 2 * np.pi / 1024  # rad per DECT sample
        if fp >= 0:
            win = F.channel(rng, x, n_rx, S, fp, cfo * 9 / 10, snr)
        else:  # the packet's first -fp samples are lost
            full = F.channel(rng, x, n_rx, S, 0, cfo * 9 / 10, snr)
            win = np.zeros_like(full)
            win[:, : S + fp] = full[:, -fp:]
        est = float(np.float32(-cfo))
        ref = O.rx(ocf, ops, win, fp, est, nid, pt)
        win.setflags(write=False)
        out.append(dict(pcc=pcc, pdc=pdc, x=x, win=win, fp=fp, est=est, nid=nid, pt=pt, ref=ref))
    return out, sz, S


@pytest.mark.parametrize("name", ["rx4_tx4", "rx4_tx2", "rx1_tx1"])
def test_tx(name):
    import dnrp
    ws, sz, S = _inputs(name)
    n_tx = sz["N_TX"]
    phy = dnrp.Phy(1, 16, n_tx, 1, 10, 9, max_batch=4)
    for w in ws:
        phy.add_network_id(w["nid"])
    ps = dnrp.psdef(*_psd(name))
    dev = torch.device("cuda:0")
    descs = [dnrp.TxDesc(0, w["nid"], w["pt"], 5, 1.0, 0.0, 0.0, 0) for w in ws]
    out = torch.full((N_PKT, n_tx, S, 2), 7.0, dtype=torch.float32, device=dev)  # every sample must be written
    phy.tx_batch(ps, descs, torch.from_numpy(np.stack([w["pcc"] for w in ws])).to(dev),
                 torch.from_numpy(np.stack([w["pdc"] for w in ws])).to(dev), out)
    phy.sync()
    iq = out.cpu().numpy().view(np.complex64)[..., 0]
    phy.close()
    for i, w in enumerate(ws):
        for a in range(n_tx):
            err = np.linalg.norm(iq[i, a] - w["x"][a]) / np.linalg.norm(w["x"][a])
            print(name, i, a, "TX relative L2 error", err)
            assert err <= 1e-4, (name, i, a, err)


def _rx(name, monkeypatch, epoch, twin):
    import dnrp
    _, _, n_rx, _ = CASES[name]
    for k in ("DNRP_RX_EPOCH", "DNRP_RX_FUSED", "DNRP_RX_SNR_FRONT", "DNRP_RX_GROUP"):
        monkeypatch.delenv(k, raising=False)
    if epoch:
        monkeypatch.setenv("DNRP_RX_EPOCH", "2")
    monkeypatch.setenv("DNRP_EQ_TWIN", "1" if twin else "0")  # read at context creation
    monkeypatch.setenv("DNRP_TIMING", "1")
    ws, sz, S = _inputs(name)
    phy = dnrp.Phy(1, 16, n_rx, 1, 10, 9, max_batch=4)
    for w in ws:
        phy.add_network_id(w["nid"])
    ps = dnrp.psdef(*_psd(name))
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack([w["win"] for w in ws]).view(np.float32).reshape(N_PKT, n_rx, S, 2)).to(dev)
    reports = [dnrp.SyncReport(w["fp"], w["est"], 0.0, 1, 16, sz["N_eff_TX"], window=i) for i, w in enumerate(ws)]
    pcc_llr = torch.zeros((N_PKT, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.full((N_PKT, sz["G"]), 0x5A5A, dtype=torch.int16, device=dev)  # every LLR must be written
    phy.rx_pcc_batch(reports, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, w["nid"], w["pt"]) for i, w in enumerate(ws)], iq, pdc_llr)
    phy.sync()
    ran_epoch = phy.kernel_time_total("rx_epoch")[1] > 0
    phy.close()
    assert ran_epoch == epoch, name
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    for i, w in enumerate(ws):
        llr_gate.check((name, i, "pcc"), g_pcc[i], w["ref"]["pcc_llr"])
        llr_gate.check((name, i, "pdc"), g_pdc[i][: len(w["ref"]["pdc_llr"])], w["ref"]["pdc_llr"])


@pytest.mark.parametrize("twin", [1, 0])
@pytest.mark.parametrize("name", ["rx4_tx4", "rx4_tx2", "rx2_tx1", "rx4_tx4_qpsk"])
def test_rx_epoch(name, twin, monkeypatch):
    _rx(name, monkeypatch, True, bool(twin))


def test_rx_y_path(monkeypatch):
    _rx("rx1_tx1", monkeypatch, False, True)
