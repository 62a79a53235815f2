"""Twin units of the epoch receiver (rx_epoch.hip / rx_eq.hpp eq_twin_first, eq_twin_second): two
consecutive symbols of one interpolation event on the same subcarriers share a unit, the channel of a
transmit stream both SFBC pairs carry is interpolated once. The sums and their order are those of two
plain units, so the LLRs must equal those of the plain plan (DNRP_EQ_TWIN=0) exactly.

Every case is a beta = 1 packet (56 subcarriers, 28 SFBC pairs per full symbol) of 6 subslots in a
u_max = 8 / b_max = 16 context, the smallest geometry the epoch receiver takes (N_b_DFT_os = 1024):
the six (N_RX, N_eff_TX) instantiations, N_bps = 8 and a run-time N_bps, stride 2 and 3 (events of three
symbols: a twin and a single) and mode l, the -5 dB and 15 dB Wiener profiles (14 / 8 taps), and a PDC
batch that drops a packet of its PCC batch. (phy_fixtures.channel sets the SNR over the whole sampled band,
of which a beta = 1 packet fills a sixteenth: the receiver's estimate, which picks the profile, lies about
11 dB above it. The profile case therefore runs at -12 dB and 0 dB, estimated -1 dB and 11 dB, and
test_profiles_of_the_snr_case asserts the picks.) Per case: the windows and the oracle's LLRs are built once,
the GPU runs twice (twin, plain); asserted are
  * pdc_llr (twin) == pdc_llr (plain), exactly,
  * the twin run against the oracle through tests/llr_gate.py,
  * that the epoch kernel ran and that its plan has twin segments (dnrp_query_table "rx_plan_segs").
"""
import functools

import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CTX = (8, 16, 1, 10, 9)  # u_max, b_max, os_min, L, M
# id: (tm_mode, mcs, N_RX, chestim lr, stride, per-packet SNR dB, PDC batch slots or None for all)
CASES = {
    "rx1_mrc_256qam": (0, 8, 1, 1, 2, (30.0, 14.0), None),
    "rx2_mrc_64qam": (0, 6, 2, 1, 2, (25.0, 12.0), None),       # run-time N_bps
    "rx4_mrc_256qam": (0, 8, 4, 1, 2, (30.0,), None),
    "rx2_txdiv2_256qam": (1, 8, 2, 1, 2, (30.0, 20.0), None),
    "rx4_txdiv2_16qam": (1, 4, 4, 1, 2, (20.0, 12.0), None),    # run-time N_bps
    "rx4_txdiv4_256qam": (5, 8, 4, 1, 2, (30.0, -12.0, 0.0), None),  # profiles 2, 0 (14 taps), 1 (8 taps)
    "rx4_txdiv4_16qam": (5, 3, 4, 1, 2, (20.0,), None),         # run-time N_bps
    "rx4_txdiv4_stride3": (5, 8, 4, 1, 3, (30.0, 12.0), None),
    "rx4_txdiv2_stride3": (1, 8, 4, 1, 3, (30.0,), None),
    "rx4_mrc_stride3": (0, 8, 4, 1, 3, (30.0,), None),
    "rx4_txdiv4_lmode": (5, 8, 4, 0, 2, (30.0, 12.0), None),
    "rx2_txdiv2_lmode": (1, 6, 2, 0, 2, (25.0,), None),
    "rx4_txdiv4_dropped": (5, 8, 4, 1, 2, (30.0, 30.0, 18.0), (0, 2)),
}


def _psd(c):
    return (8, 1, 0, 6, c[0], c[1])


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The case's windows, sync report fields and the oracle's PDC LLRs, built once."""
    tm, mcs, n_rx, lr, stride, snrs, _ = CASES[name]
    u_max, b_max, os_min, L, M = CTX
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M, lr=lr, stride=stride), O.psdef(*_psd(CASES[name]))
    sz = O.packet_sizes(ops)
    d = O.dims(ocf, ops)
    S, n_dft = d["N_packet_os_rs"], d["N_b_DFT_os"]
    rng = np.random.default_rng(0x7E1)
    out = []
    for i, snr in enumerate(snrs):
        pcc, pdc = O.pack_bits(F.random_bits(rng, 196)), O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + i, 1 + i % 2
        iq_tx, _ = O.tx(ocf, ops, pcc, pdc, S, network_id=nid, plcf_type=pt)
        off = int(rng.integers(0, 32))
        cfo = rng.uniform(-1.75, 1.75) * 2 * np.pi / n_dft  # rad per DECT sample
        win = F.channel(rng, iq_tx, n_rx, S, off, cfo * M / L, snr)
        est = float(np.float32(-cfo + rng.uniform(-0.02, 0.02) * 2 * np.pi / n_dft))
        ref = O.rx(ocf, ops, win, off, est, nid, pt)
        win.setflags(write=False)
        out.append(dict(win=win, off=off, est=est, nid=nid, pt=pt, ref=ref["pdc_llr"], picks=ref["lut_picks"]))
    return out


def _gpu_pdc(name, twin, monkeypatch):
    import dnrp
    tm, mcs, n_rx, lr, stride, snrs, slots = CASES[name]
    u_max, b_max, os_min, L, M = CTX
    monkeypatch.setenv("DNRP_EQ_TWIN", "1" if twin else "0")  # read at context creation
    monkeypatch.setenv("DNRP_RX_EPOCH", "2")
    monkeypatch.setenv("DNRP_TIMING", "1")
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, chestim_mode_lr=bool(lr), stride=stride, max_batch=8)
    ws = _inputs(name)
    for w in ws:
        phy.add_network_id(w["nid"])
    ps = dnrp.psdef(*_psd(CASES[name]))
    sz = phy.packet_sizes(ps)
    assert sz["N_b_DFT_os"] == 1024 and sz["N_b_OCC"] == 56
    dev = torch.device("cuda:0")
    n, S = len(ws), sz["N_samples_packet_os_rs"]
    iq = torch.from_numpy(np.stack([w["win"] for w in ws]).view(np.float32).reshape(n, n_rx, S, 2)).to(dev)
    reports = [dnrp.SyncReport(w["off"], w["est"], 0.0, 8, 1, sz["N_eff_TX"]) for w in ws]
    slots = tuple(range(n)) if slots is None else slots
    pcc_llr = torch.zeros((n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.full((len(slots), sz["G"]), 0x5A5A, dtype=torch.int16, device=dev)  # every LLR must be written
    phy.rx_pcc_batch(reports, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, ws[i]["nid"], ws[i]["pt"]) for i in slots], iq, pdc_llr)
    phy.sync()
    assert phy.kernel_time_total("rx_epoch")[1] > 0, name
    phy.close()
    return pdc_llr.cpu().numpy(), slots, sz


def _plan_twins(name, sz):
    import dnrp
    _, _, _, lr, stride, _, _ = CASES[name]
    segs = dnrp.query_table("rx_plan_segs", 1, sz["N_TS"], sz["N_eff_TX"], sz["N_DF_symb"], lr, stride, 1)
    segs = segs.astype(np.int64).reshape(-1, 12)
    return segs[segs[:, 11] > 0], segs[segs[:, 11] == 0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_plain(name, monkeypatch):
    g_twin, slots, sz = _gpu_pdc(name, True, monkeypatch)
    g_plain, _, _ = _gpu_pdc(name, False, monkeypatch)
    twins, plains = _plan_twins(name, sz)
    assert len(twins) > 0, "the case's plan has twin segments: the twin path ran"
    if "stride3" in name:  # an event of three full symbols: a twin and a single of the same cell count
        n_full = sz["N_b_OCC"]
        assert np.any(twins[:, 11] == n_full) and np.any(plains[:, 4] - plains[:, 3] == n_full)
    assert np.array_equal(g_twin, g_plain), (name, int(np.count_nonzero(g_twin != g_plain)))
    ws = _inputs(name)
    for row, i in enumerate(slots):
        llr_gate.check((name, i, "pdc"), g_twin[row], ws[i]["ref"])


def test_profiles_of_the_snr_case():
    """Packets 1 and 2 of rx4_txdiv4_256qam run the 14- and 8-tap windows (profiles 0 and 1) at every DRS
    operation, packet 0 the 3-tap ones (from the oracle alone)."""
    ws = _inputs("rx4_txdiv4_256qam")
    for w, prof in zip(ws, (2, 0, 1)):
        assert len(w["picks"]) > 0 and {p for p, _ in w["picks"]} == {prof}, w["picks"]
