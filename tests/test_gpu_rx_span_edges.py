"""RX front end at the edges of a window row: spans that begin before the row, end past it, or sit in
the last (window, antenna) row of the allocation.

The wave front end (rx_fft_wave_ct_kernel, and the front-end phase of rx_epoch_kernel) stages a symbol's
input span through a buffer descriptor over the row's valid samples; the hardware range check supplies
the zeros outside them. A descriptor with a wrong base or range reads a neighbouring row, or memory past
the buffer for the last row. mu = 8, beta = 16, MCS 8 in one slot: 4 x 4 TM5 (rx_epoch_kernel<4, 4, 8>)
and N_RX = N_TX = 1 (the standalone front end), a batch of 8 packets each through rx_pcc_batch and
rx_pdc_batch with given sync reports, every packet against the oracle under tests/llr_gate.py.

Placements (D = the guard interval behind the packet, the window being one packet long):
  0, 1  fine peak 0 and 5: below the resampler's half-length 24, the packet's first span (the STF's)
        starts before sample 0 of the row
  2     fine peak -3: the packet starts before the window (its first 3 samples are lost)
  3     fine peak 17: every span inside the row
  4     fine peak D - 12: the last symbol's span (24 samples of filter tail) ends 12 samples past the row
  5     fine peak D: the packet's last sample is the row's last, the whole filter tail past it
  6, 7  fine peak D + 8: the last symbol loses 8 samples; packet 7 sits in the last rows of the buffer
Every row holds another packet's samples at full power, so a read that leaves its row shows in the LLRs.

Chosen on the CPU from the oracle alone: its float path stays inside the gate against its double path
for every one of these windows (max |delta| 1, at most 0.22 % of a row's PDC LLRs differing, at most one
of a PCC row's 196), so the truncated spans leave the rows well conditioned. The draw (SEED) is part of
that choice: some SISO channel and noise draws take the oracle's own float path past 1 % of a row with
no truncation at all (placement 1 at seeds 0x5BA9 and 3), and a row like that cannot gate a kernel.
"""
import functools

import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SNR_DB = 30.0
SEED = 1


def placements(D):
    return [0, 5, -3, 17, D - 12, D, D + 8, D + 8]


@functools.lru_cache(maxsize=None)
def build(name):
    """Windows, sync-report inputs and the oracle's results of configuration `name`, computed once."""
    psd, cft = F.CONFIGS[name]
    u_max, b_max, n_ant, os_min, L, M = cft
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M), O.psdef(*psd)
    sz, dm = O.packet_sizes(ops), O.dims(ocf, ops)
    S, keep = dm["N_packet_os_rs"], dm["N_no_GI_os_rs"]
    rng = np.random.default_rng(SEED)
    wins, peaks, cfos, nids, types, refs = [], [], [], [], [], []
    for i, fp in enumerate(placements(S - keep)):
        nid, pt = 100 + i % 6, 1 + i % 2
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        x, _ = O.tx(ocf, ops, pcc, pdc, S, network_id=nid, plcf_type=pt)
        cfo_dect = rng.uniform(-1.0, 1.0) * 2 * np.pi / dm["N_b_DFT_os"]
        if fp >= 0:
            win = F.channel(rng, x, n_ant, S, fp, cfo_dect * M / L, SNR_DB)
        else:  # the packet starts -fp samples before the window
            full = F.channel(rng, x, n_ant, S, 0, cfo_dect * M / L, SNR_DB)
            win = np.zeros_like(full)
            win[:, : S + fp] = full[:, -fp:]
        cfo = float(np.float32(-cfo_dect))
        wins.append(win)
        peaks.append(fp)
        cfos.append(cfo)
        nids.append(nid)
        types.append(pt)
        refs.append(O.rx(ocf, ops, win, fp, cfo, nid, pt))
    return dict(cft=cft, psd=psd, sz=sz, S=S, keep=keep, wins=wins, peaks=peaks, cfos=cfos, nids=nids, types=types, refs=refs)


@pytest.mark.parametrize("name", ["C4", "C3"])
def test_rx_span_edges(name, monkeypatch):
    import dnrp
    monkeypatch.delenv("DNRP_RX_EPOCH", raising=False)  # the default: epoch receiver with 4 antennas, Y path for 1
    monkeypatch.delenv("DNRP_RX_FUSED", raising=False)
    monkeypatch.setenv("DNRP_TIMING", "1")
    c = build(name)
    u_max, b_max, n_ant, os_min, L, M = c["cft"]
    phy = dnrp.Phy(u_max, b_max, n_ant, os_min, L, M, max_batch=8)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    ps, sz, S = dnrp.psdef(*c["psd"]), c["sz"], c["S"]
    n = len(c["wins"])
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack(c["wins"]).view(np.float32).reshape(n, n_ant, S, 2)).to(dev)
    assert c["peaks"][n - 1] + c["keep"] > S  # the packet in the buffer's last rows runs past their end
    assert phy.packet_sizes(ps)["N_samples_packet_os_rs"] == S
    reports = [dnrp.SyncReport(c["peaks"][i], c["cfos"][i], 0.0, c["psd"][0], c["psd"][1], sz["N_eff_TX"], window=i)
               for i in range(n)]
    pcc_llr = torch.zeros((n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((n, sz["G"]), dtype=torch.int16, device=dev)
    phy.rx_pcc_batch(reports, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, c["nids"][i], c["types"][i]) for i in range(n)], iq, pdc_llr)
    phy.sync()
    assert (phy.kernel_time_total("rx_epoch")[1] > 0) == (n_ant == 4), name
    g_pcc, g_pdc = pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy()
    for i, r in enumerate(c["refs"]):
        llr_gate.check((name, "edge", i, "pcc"), g_pcc[i], r["pcc_llr"])
        llr_gate.check((name, "edge", i, "pdc"), g_pdc[i][: len(r["pdc_llr"])], r["pdc_llr"])
