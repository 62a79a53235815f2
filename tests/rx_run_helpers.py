"""What the GPU tests of the receiver's context settings share (test_gpu_rx_sto_track.py, test_gpu_rx_cfo_track.py,
test_gpu_rx_mimo_report.py; TEST INFRASTRUCTURE): a clean environment with the kernel timers on, a context with the
tests' network ids, one PCC batch and one PDC batch with the read-backs a test asks for, and report equality."""
import collections

import numpy as np

ENV = ("DNRP_RX_EPOCH", "DNRP_RX_FUSED", "DNRP_RX_SNR_FRONT", "DNRP_RX_GROUP")

RxRun = collections.namedtuple("RxRun", "pcc_llr pdc_llr rep1 rep2 cfo_tab sto_tab rows")


def clean_env(monkeypatch, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DNRP_TIMING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def phy(ctx, lr=1, max_batch=4):
    import dnrp
    u_max, b_max, n_rx, os_min, L, M = ctx
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, chestim_mode_lr=bool(lr), max_batch=max_batch)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    return phy


def rx(phy, psd, windows, reports, reqs, pcc_report=True, pdc_report=True, cfo_table=False, sto_table=False, detail=False):
    """One PCC batch of all windows and one PDC batch of reqs = [(pcc_index, network_id, plcf_type)]: the LLRs
    (torch, host), the reports (None where not asked for), the CFO and STO tables and the MIMO detail rows or None"""
    import dnrp
    import torch
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    n, n_rx, S = len(windows), phy.cfg.N_TX_max, windows[0].shape[1]
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack(windows).view(np.float32).reshape(n, n_rx, S, 2)).to(dev)
    pcc_llr = torch.zeros((n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((len(reqs), sz["G"]), dtype=torch.int16, device=dev)
    rep1 = phy.rx_pcc_batch(reports, iq, pcc_llr, want_report=pcc_report)
    rep2 = phy.rx_pdc_batch([dnrp.PdcReq(ps, i, nid, pt) for i, nid, pt in reqs], iq, pdc_llr, want_report=pdc_report)
    phy.sync()
    cfo_tab = phy.rx_cfo_track(n) if cfo_table else None
    sto_tab = phy.rx_sto_track(n) if sto_table else None
    rows = phy.rx_mimo_detail(len(reqs)) if detail else None
    return RxRun(pcc_llr.cpu(), pdc_llr.cpu(), rep1, rep2, cfo_tab, sto_tab, rows)


def same_pcc_reports(a, b):
    for x, y in zip(a, b):
        assert (x.snr_dB, x.cfo_fractional_rad, x.sto_fractional, list(x.rms)) == \
            (y.snr_dB, y.cfo_fractional_rad, y.sto_fractional, list(y.rms))


def same_pdc_reports(a, b):
    for x, y in zip(a, b):
        assert (x.snr_dB, x.mimo_N_RX, x.mimo_N_TS_other, x.tm_3_7_beamforming_idx, x.tm_3_7_beamforming_reciprocal_idx) == \
            (y.snr_dB, y.mimo_N_RX, y.mimo_N_TS_other, y.tm_3_7_beamforming_idx, y.tm_3_7_beamforming_reciprocal_idx)
