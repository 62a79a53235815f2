"""Device pins of the DRS / PCC / PDC cell maps: the TX kernels' grid and the receivers' cell order
against tests/golden/ref_cells.json (the reference's compiled drs.cpp / pcc.cpp / pdc.cpp), never
against the oracle.

Contexts have u_max = 1, b_max = b, os_min = 1 and L = M = 1, so the TX output is the OFDM symbols
themselves: stripping the CP and one numpy FFT per symbol recovers the grid per antenna (lengths from
the pinned numerologies / packet_structure of ref_tables.json). Packets are u = 1, PacketLengthType 1,
PacketLength 3 (N_DF = 28 >= 22: the 10-symbol PDC repetition is exercised), codebook 0 (pinned W: one
non-zero entry per row, antenna = stream), zero phase and increment.

Positions. The fixture holds full index lists for b <= 2 and count + SHA-256 digest above; the lists used
here are the host maps after they matched the fixture entry by entry (_positions), so every expectation
is the fixture's. With A the RMS magnitude of the data cells: every bin outside the fixture's cells
(guards, DC, other streams' DRS cells, unused symbols) <= 1e-3 A (exact zeros cost ~1e-6 through a float
IFFT / FFT pair; 1e-3 is 100x below any real cell); DRS cells carry the fixture's +-1 values relative to
stream 0's first DRS cell within 1e-3 (streams 4..7 negated, as y_DRS_i says); every PCC / PDC position
>= 0.1 A on the streams that carry it and <= 1e-3 A on the others.

Order, by differential flips (scrambling is an XOR, so no Gold sequence or modulation table is needed):
packet 0 carries random d-bits, packet 1 + q flips all N_bps bits of every PDC (and PCC) d-symbol whose
index has bit q set, the last packet flips every symbol. A grid entry changed when |dX| >= 0.1 A and did
not when |dX| <= 1e-3 A; nothing may lie between (a full flip moves a QPSK cell by 2 A and a 256-QAM cell
by >= 2 / sqrt(170) = 0.153 A). The packets in which an entry changed spell the d-symbol index it
carries. SISO: position j carries index j. Transmit diversity (tx.cpp:961-973 PCC, 1090-1103 PDC): cell j
belongs to pair j / 2, whose streams (A, B) are row (j / 2) % modulo of Y_i_t::index_N_TS_x (pinned
"txdiv_pairs"); stream A carries symbol j (tx.cpp:969, 1098), stream B the flipped partner j ^ 1
(tx.cpp:970, 1099), every other stream nothing.

RX order (N_eff_TX <= 4; 8 stays DNRP_EUNSUPPORTED, test_rx_tm10_unsupported): the same GPU-TX packets
pass noiselessly through a seeded random H (N_RX = N_TX_max, zero CFO, offset in [0, 32)) into
rx_pcc_batch / rx_pdc_batch; the hard decisions equal the transmitted bits exactly, for every packet.
The TX half has pinned positions and order absolutely, so an exact loopback pins the receivers' order.
The bar is no stricter than the restatement: test_oracle_loopback_error_free (CPU, not gpu) runs the
oracle TX and RX on windows built by the same code and requires zero bit errors at every geometry.
DNRP_RX_EPOCH=0 / 2 and DNRP_RX_FUSED=1 are run at b in {1, 4, 16} x TM in {0, 5}: in these L = M = 1
contexts the epoch and fused receivers do not apply (they need the 10/9 wave front end,
rx.cpp choose_pdc_path), so their launch counts must be 0 and the Y path must still be exact; in a
10/9 context at b = 16 (N_b_DFT_os = 1024), where they do apply, the same loopback runs through them
with the launch count proving it.
"""
import functools
import json
import os

import numpy as np
import pytest

import cell_fixture as CF
import oracle_py as O
import phy_fixtures as F

RT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tables.json")))
LIT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_literals.json")))

U, PLT, PL = 1, 1, 3
N_TS_OF_TM = {0: 1, 1: 2, 5: 4, 10: 8}  # SISO and the transmit-diversity modes (tm_mode.cpp:27-137)
NID, PLCF_TYPE = 100, 1
# (b, tm, mcs): QPSK over the grid, plus one 256-QAM and one 64-QAM case for the multi-bit byte paths
QPSK_GEOMS = [(b, tm, 1) for b in (1, 2, 4, 8, 12, 16) for tm in (0, 1, 5, 10)]
QAM_GEOMS = [(16, 5, 8), (4, 0, 6)]
TX_GEOMS = QPSK_GEOMS + QAM_GEOMS
RX_GEOMS = [g for g in TX_GEOMS if N_TS_OF_TM[g[1]] <= 4]
SWITCH_GEOMS = [(b, tm, 1) for b in (1, 4, 16) for tm in (0, 5)]
_id = lambda g: f"b{g[0]}_tm{g[1]}_mcs{g[2]}"  # noqa: E731


# ---------------------------------------------------------------- pinned lengths and positions
def _lengths(b):
    """(N_b_DFT, CP, guards_bottom, STF, symbol, N_DF) of a u = 1 packet, all from compiled reference code"""
    num = next(r for r in RT["numerologies"] if r["u"] == U and r["b"] == b)
    st = next(r for r in RT["packet_structure"] if r["u"] == U and r["b"] == b and r["PLT"] == PLT)
    n_df = CF.counts("N_DF_symb")[1][(U, PLT, PL)]
    assert st["sym"] == num["N_b_DFT"] + num["N_b_CP"]
    return num["N_b_DFT"], num["N_b_CP"], num["N_guards_bottom"], st["STF"], st["sym"], n_df


def _positions(b, n_ts, n_df):
    """PCC (l, k) rows, PDC (l, k) rows in mapping order and DRS rows (l, ts_first, ts_last, k, y) of the
    host maps, each matched against the fixture (list or count + digest) before it is used"""
    import dnrp
    g = CF.geometry(b, n_ts)
    pcc = dnrp.pcc_cells(b, n_ts)
    assert len(pcc) == 98 and sorted(set(pcc[:, 0].tolist())) == g["pcc"]["l"]
    for l, idx in zip(g["pcc"]["l"], g["pcc"]["k"]):
        assert CF.matches(idx, pcc[pcc[:, 0] == l, 1]), ("PCC", b, n_ts, l)
    pdc = dnrp.pdc_cells(b, n_ts, n_df)
    assert pdc[:, 0].tolist() == sorted(pdc[:, 0].tolist())
    for l in range(1, n_df + 1):
        assert CF.matches(g["pdc"][l - 1], pdc[pdc[:, 0] == l, 1]), ("PDC", b, n_ts, l)
    want = [r for r in g["drs"] if r[0] <= n_df]
    got = dnrp.drs_cells(b, n_ts, n_df)
    assert [r[:3] for r in got] == [tuple(r[:3]) for r in want]
    drs = []
    for (l, first, last, k), row in zip(got, want):
        for s in range(last - first + 1):
            assert CF.matches(row[3][s], k[s]), ("DRS", b, n_ts, l, first + s)
        drs.append((l, first, last, k, np.stack([CF.bits(i) for i in row[4]])))
    return pcc, pdc, drs


def _stream_of_antenna(n_ts):
    """codebook 0 of the pinned compiled W_t: one non-zero entry per row, so antenna = stream (scaled)"""
    e = next(w for w in CF.GOLD["W"] if w["N_TS"] == n_ts and w["N_TX"] == n_ts and w["codebook"] == 0)
    w = np.array(e["W"], np.float64).view(np.complex128).reshape(n_ts, n_ts)
    assert ((w != 0).sum(axis=1) == 1).all() and ((w != 0).sum(axis=0) == 1).all()
    return np.argmax(w != 0, axis=1), w[w != 0]


def _txdiv_pairs(n_ts):
    row = {2: 0, 4: 1, 8: 2}[n_ts]
    pairs = np.array(LIT["index_N_TS_x"][row])
    assert len(pairs) == LIT["txdiv_modulo"][str(n_ts)]
    return pairs


# ---------------------------------------------------------------- packets
def _packets(b, tm, mcs, seed=0xCE11):
    """d-bits of the flip packets: (pcc bits [n, 196], pdc bits [n, G], number of index bits)"""
    n_pdc = CF.counts("N_PDC_subc")[1][(U, b, PLT, PL, N_TS_OF_TM[tm])]
    n_bps = next(m["N_bps"] for m in RT["mcs"] if m["index"] == mcs)
    nb = max(int(n_pdc - 1).bit_length(), 7)  # 98 PCC symbols need 7
    rng = np.random.default_rng(seed)
    pcc0, pdc0 = F.random_bits(rng, 196), F.random_bits(rng, n_pdc * n_bps)
    j_pcc, j_pdc = np.repeat(np.arange(98), 2), np.repeat(np.arange(n_pdc), n_bps)
    pcc, pdc = [pcc0], [pdc0]
    for q in range(nb):
        pcc.append(pcc0 ^ ((j_pcc >> q) & 1).astype(np.uint8))
        pdc.append(pdc0 ^ ((j_pdc >> q) & 1).astype(np.uint8))
    pcc.append(pcc0 ^ 1)
    pdc.append(pdc0 ^ 1)
    return np.stack(pcc), np.stack(pdc), nb


def _pack(bits):
    return np.stack([O.pack_bits(r) for r in bits])


def _windows(iq, n_rx, seed=0x0FF5):
    """noiseless windows of the packets iq [n, N_TX, S] through one seeded random H, zero CFO, a seeded
    offset in [0, 32) per packet (the tail cut off by the offset is guard interval)"""
    rng = np.random.default_rng(seed)
    H = F.mixing_matrix(rng, n_rx, iq.shape[1])
    offs = [int(rng.integers(0, 32)) for _ in range(iq.shape[0])]
    return [F.channel(rng, iq[i], n_rx, iq.shape[2], offs[i], 0.0, None, H=H) for i in range(iq.shape[0])], offs


# ---------------------------------------------------------------- grid checks (source-agnostic)
def _grids(iq, b):
    """iq [n, N_ant, S] complex64 -> per packet the fftshifted grid [n, N_stream, N_DF, N_b_DFT]"""
    N, cp, _, stf, sym, n_df = _lengths(b)
    stream, w = _stream_of_antenna(iq.shape[1])
    out = np.empty((iq.shape[0], iq.shape[1], n_df, N), np.complex64)
    for p in range(iq.shape[0]):
        x = iq[p][:, stf:stf + n_df * sym].reshape(iq.shape[1], n_df, sym)[:, :, cp:]
        X = np.fft.fftshift(np.fft.fft(x, axis=-1), axes=-1)
        out[p][stream] = X / w[:, None, None]
    return out


def _check_grid(G, b, tm, nb):
    """G: grids of the flip packets [2 + nb, N_TS, N_DF, N_b_DFT]"""
    n_ts = N_TS_OF_TM[tm]
    N, _, gb, _, _, n_df = _lengths(b)
    pcc, pdc, drs = _positions(b, n_ts, n_df)
    assert G.shape == (nb + 2, n_ts, n_df, N)
    X0 = G[0]
    data = np.concatenate([pcc, pdc])
    dl, di = data[:, 0] - 1, data[:, 1] + gb
    assert len(set(zip(dl.tolist(), di.tolist()))) == len(data)  # no position twice
    # A: RMS magnitude of the data cells (one stream carries a SISO cell, two an SFBC cell)
    A = float(np.sqrt((np.abs(X0[:, dl, di]).astype(np.float64) ** 2).sum() / (len(data) * (1 if n_ts == 1 else 2))))
    assert A > 0
    # --- positions: DRS values, then everything that is neither DRS nor data must be empty
    free = np.ones(X0.shape, bool)
    free[:, dl, di] = False
    ref = None
    for l, first, last, k, y in drs:
        for s, t in enumerate(range(first, last + 1)):
            v = X0[t, l - 1, k[s] + gb]
            if ref is None:
                ref = v[0] / y[s][0]
                assert abs(ref) >= 0.1 * A, (b, tm, "DRS reference cell empty")
            err = np.abs(v / ref - y[s])
            assert err.max() <= 1e-3, (b, tm, "DRS value", l, t, int(err.argmax()), float(err.max()))
            free[t, l - 1, k[s] + gb] = False
    stray = np.abs(X0) * free
    assert stray.max() <= 1e-3 * A, (b, tm, "occupied outside the fixture's cells",
                                     np.unravel_index(int(stray.argmax()), stray.shape), float(stray.max() / A))
    # --- differential flips
    D = np.abs(G[1:] - X0[None])
    chg, unchg = D >= 0.1 * A, D <= 1e-3 * A
    assert (chg | unchg).all(), (b, tm, "change between the thresholds", float(D[~(chg | unchg)].min() / A))
    assert not chg[:, free].any() and not chg[:, ~free & (np.abs(X0) <= 1e-3 * A)].any(), (b, tm, "empty cell moved")
    for l, first, last, k, _ in drs:
        for s, t in enumerate(range(first, last + 1)):
            assert not chg[:, t, l - 1, k[s] + gb].any(), (b, tm, "DRS cell moved", l, t)
    idx = np.zeros(X0.shape, np.int64)
    for q in range(nb):
        idx |= chg[q].astype(np.int64) << q
    allflip = chg[nb]
    mag = np.abs(X0)
    for name, cells in (("PCC", pcc), ("PDC", pdc)):
        cl, ci, j = cells[:, 0] - 1, cells[:, 1] + gb, np.arange(len(cells))
        m = mag[:, cl, ci]  # [N_TS, cells]
        top = m.max(axis=0)
        assert (top >= 0.1 * A).all(), (b, tm, name, "empty position", int((top < 0.1 * A).argmax()))
        carried = np.zeros(m.shape, bool)
        if n_ts == 1:
            carried[0] = True
            assert np.array_equal(idx[0, cl, ci], j), (b, tm, name, "order", int((idx[0, cl, ci] != j).argmax()))
        else:
            assert len(cells) % 2 == 0
            pairs = _txdiv_pairs(n_ts)
            sa, sb = pairs[(j // 2) % len(pairs)].T
            carried[sa, j] = carried[sb, j] = True
            ia, ib = idx[sa, cl, ci], idx[sb, cl, ci]
            assert np.array_equal(ia, j), (b, tm, name, "stream A order", int((ia != j).argmax()))
            assert np.array_equal(ib, j ^ 1), (b, tm, name, "stream B order", int((ib != (j ^ 1)).argmax()))
        assert (m[carried] >= 0.1 * A).all() and (m[~carried] <= 1e-3 * A).all(), (b, tm, name, "streams of a cell")
        assert allflip[:, cl, ci][carried].all(), (b, tm, name, "all-flip packet left a data entry unchanged")
        assert not chg[:, :, cl, ci].transpose(1, 2, 0)[~carried].any(), (b, tm, name, "flip reached another stream")
    return A


def _check_hard(pcc_llr, pdc_llr, pcc_bits, pdc_bits, tag):
    for i in range(len(pcc_bits)):
        e1 = int(np.sum((pcc_llr[i] > 0).astype(np.uint8) != pcc_bits[i]))
        e2 = int(np.sum((pdc_llr[i][: pdc_bits.shape[1]] > 0).astype(np.uint8) != pdc_bits[i]))
        assert e1 == 0 and e2 == 0, (tag, "packet", i, "PCC bit errors", e1, "PDC bit errors", e2)


# ---------------------------------------------------------------- CPU: the bar is no stricter than the oracle
def _oracle_tx(b, tm, mcs, L=1, M=1):
    pcc_bits, pdc_bits, nb = _packets(b, tm, mcs)
    cf, ps = O.cfg(U, b, 1, L, M), O.psdef(U, b, PLT, PL, tm, mcs)
    S = O.dims(cf, ps)["N_packet_os_rs"]
    pcc, pdc = _pack(pcc_bits), _pack(pdc_bits)
    iq = np.stack([O.tx(cf, ps, pcc[i], pdc[i], S, codebook=0, network_id=NID, plcf_type=PLCF_TYPE)[0]
                   for i in range(len(pcc))])
    return iq, pcc_bits, pdc_bits, nb, cf, ps


RESAMPLED_GEOMS = [(16, 0, 1, 10, 9), (16, 5, 1, 10, 9)]  # (b, tm, mcs, L, M)


@pytest.mark.parametrize("geom", RX_GEOMS + RESAMPLED_GEOMS, ids=lambda g: _id(g) + ("_lm10_9" if len(g) > 3 else ""))
def test_oracle_loopback_error_free(geom):
    """the condition of the GPU loopback below: oracle TX -> the same windows -> oracle RX, zero bit errors"""
    b, tm, mcs = geom[:3]
    L, M = geom[3:] if len(geom) > 3 else (1, 1)
    iq, pcc_bits, pdc_bits, _, cf, ps = _oracle_tx(b, tm, mcs, L, M)
    wins, offs = _windows(iq, N_TS_OF_TM[tm])
    rx = [O.rx(cf, ps, wins[i], offs[i], 0.0, NID, PLCF_TYPE) for i in range(len(wins))]
    _check_hard([r["pcc_llr"] for r in rx], [r["pdc_llr"] for r in rx], pcc_bits, pdc_bits, geom)


@pytest.mark.parametrize("geom", [(1, 0, 1), (1, 5, 1), (2, 1, 1), (2, 10, 1)], ids=_id)
def test_oracle_tx_grid(geom):
    """the grid and flip checks themselves, run on the oracle's TX on the CPU: the analysis accepts a
    correct transmitter, and the oracle's TX is pinned to the fixture absolutely at these geometries"""
    b, tm, mcs = geom
    iq, _, _, nb, _, _ = _oracle_tx(b, tm, mcs)
    _check_grid(_grids(iq, b), b, tm, nb)


def test_grid_check_rejects_swapped_cells():
    """a transmitter that swaps two PDC cells of one symbol, or moves a DRS cell, fails the checks"""
    b, tm, mcs = 1, 0, 1
    iq, _, _, nb, _, _ = _oracle_tx(b, tm, mcs)
    G = _grids(iq, b)
    _, _, gb, _, _, n_df = _lengths(b)
    _, pdc, drs = _positions(b, 1, n_df)
    bad = G.copy()
    (l0, k0), (l1, k1) = pdc[200], pdc[201]
    bad[:, 0, l0 - 1, k0 + gb], bad[:, 0, l1 - 1, k1 + gb] = G[:, 0, l1 - 1, k1 + gb], G[:, 0, l0 - 1, k0 + gb]
    with pytest.raises(AssertionError, match="order"):
        _check_grid(bad, b, tm, nb)
    bad = G.copy()
    l, _, _, k, _ = drs[1]
    bad[:, 0, l - 1, k[0][3] + gb + 1] += bad[:, 0, l - 1, k[0][3] + gb]
    bad[:, 0, l - 1, k[0][3] + gb] = 0
    with pytest.raises(AssertionError, match="DRS value"):
        _check_grid(bad, b, tm, nb)


# ---------------------------------------------------------------- GPU
def _phy(b, n_ant, n, L=1, M=1):
    import dnrp
    phy = dnrp.Phy(U, b, n_ant, 1, L, M, max_batch=n)
    phy.add_network_id(NID)
    return phy


@functools.lru_cache(maxsize=2)
def _gpu_tx(b, tm, mcs, L=1, M=1):
    """the flip packets through dnrp_tx_batch: (iq [n, N_TX, S] complex64, pcc bits, pdc bits, nb)"""
    import dnrp
    import torch
    pcc_bits, pdc_bits, nb = _packets(b, tm, mcs)
    n = len(pcc_bits)
    phy = _phy(b, N_TS_OF_TM[tm], n, L, M)
    ps = dnrp.psdef(U, b, PLT, PL, tm, mcs)
    sz = phy.packet_sizes(ps)
    assert sz["G"] == pdc_bits.shape[1] and sz["N_TX"] == N_TS_OF_TM[tm]
    S = sz["N_samples_packet_os_rs"]
    dev = torch.device("cuda:0")
    out = torch.full((n, sz["N_TX"], S, 2), 7.0, dtype=torch.float32, device=dev)
    descs = [dnrp.TxDesc(0, NID, PLCF_TYPE, 5, 1.0, 0.0, 0.0, 0) for _ in range(n)]
    phy.tx_batch(ps, descs, torch.from_numpy(_pack(pcc_bits)).to(dev), torch.from_numpy(_pack(pdc_bits)).to(dev), out)
    phy.sync()
    iq = out.cpu().numpy().view(np.complex64)[..., 0]
    phy.close()
    return iq, pcc_bits, pdc_bits, nb


def _gpu_loopback(b, tm, mcs, L=1, M=1):
    """GPU TX -> seeded noiseless windows -> GPU RX, exact hard decisions; returns the RX context"""
    import dnrp
    import torch
    iq, pcc_bits, pdc_bits, _ = _gpu_tx(b, tm, mcs, L, M)
    n, n_rx = len(iq), N_TS_OF_TM[tm]
    wins, offs = _windows(iq, n_rx)
    phy = _phy(b, n_rx, n, L, M)
    ps = dnrp.psdef(U, b, PLT, PL, tm, mcs)
    dev = torch.device("cuda:0")
    win = torch.from_numpy(np.stack(wins).view(np.float32).reshape(n, n_rx, iq.shape[2], 2)).to(dev)
    pcc_llr = torch.zeros((n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((n, pdc_bits.shape[1]), dtype=torch.int16, device=dev)
    phy.rx_pcc_batch([dnrp.SyncReport(offs[i], 0.0, 0.0, U, b, n_rx) for i in range(n)], win, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, NID, PLCF_TYPE) for i in range(n)], win, pdc_llr)
    phy.sync()
    _check_hard(pcc_llr.cpu().numpy(), pdc_llr.cpu().numpy(), pcc_bits, pdc_bits, (b, tm, mcs, L, M))
    return phy


@pytest.mark.gpu
@pytest.mark.parametrize("geom", TX_GEOMS, ids=_id)
def test_tx_grid(geom):
    b, tm, mcs = geom
    iq, _, _, nb = _gpu_tx(b, tm, mcs)
    N, _, _, stf, sym, n_df = _lengths(b)
    assert np.all(iq[:, :, stf + n_df * sym:] == 0), "guard interval not zero"
    _check_grid(_grids(iq, b), b, tm, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", RX_GEOMS, ids=_id)
def test_rx_order(geom):
    _gpu_loopback(*geom).close()


SWITCHES = {"ypath": ("DNRP_RX_EPOCH", "0"), "epoch": ("DNRP_RX_EPOCH", "2"), "fused": ("DNRP_RX_FUSED", "1")}


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("geom", SWITCH_GEOMS, ids=_id)
def test_rx_order_switches(geom, switch, monkeypatch):
    """L = M = 1: neither the epoch nor the fused receiver applies (no 10/9 wave front end); the switch
    must fall back to the Y path, which stays exact"""
    monkeypatch.setenv(*SWITCHES[switch])
    monkeypatch.setenv("DNRP_TIMING", "1")
    phy = _gpu_loopback(*geom)
    assert phy.kernel_time_total("rx_epoch")[1] == 0 and phy.kernel_time_total("rx_fused")[1] == 0, (geom, switch)
    assert phy.kernel_time_total("rx_pdc")[1] > 0, (geom, switch)
    phy.close()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("tm", [0, 5])
def test_rx_order_switches_resampled_b16(tm, switch, monkeypatch):
    """b = 16 in a 10/9 context (N_b_DFT_os = 1024), where the epoch and the fused receiver apply: the same
    exact loopback through each of them, the launch counts proving which receiver ran"""
    monkeypatch.setenv(*SWITCHES[switch])
    monkeypatch.setenv("DNRP_TIMING", "1")
    phy = _gpu_loopback(16, tm, 1, 10, 9)
    n_ep, n_fu = phy.kernel_time_total("rx_epoch")[1], phy.kernel_time_total("rx_fused")[1]
    assert (n_ep > 0, n_fu > 0) == {"ypath": (False, False), "epoch": (True, False), "fused": (False, True)}[switch], \
        (tm, switch, n_ep, n_fu)
    phy.close()
