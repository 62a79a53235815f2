"""The streaming TX kernel's one-hot code table (csrc/host/tables.cpp tx_code_oh, kernels.hpp OH_*) as
get_tx uploads it, read through dnrp_query_table "tx_code_oh", against a numpy restatement built from the
cell maps ("symbol_cells", "pdc_cells", "pcc_cells", "drs_cells", "drs_values", "stf") and the SFBC pair
schedule ("txdiv_pairs"). No GPU.

A DF bin's word says where the kernel finds the bin's bits and which constellation slot they select:
  BO  byte offset from the symbol's first staged byte   SH, WD  the bit field in the big-endian byte pair at BO
  K   XORed into the field: the SFBC partner's sign flip as the index bit that carries the sign, or the slot of
      a value that is no PDC point (256, 257: DRS +1 / -1, 258: empty, 260..263: the PCC's QPSK points,
      264.. / 266..: BPSK with re / im flipped)
"""
import numpy as np
import pytest

import tx_stream_edge_cases as E

PCB, ZB = 9280, 9280 + 25  # the wave's descrambled PCC bytes, and a zero byte behind them
Q_DRS, Q_ZERO, Q_QPSK, Q_BPSK_FX, Q_BPSK_FY = 256, 258, 260, 264, 266


def _slot(k, N):
    """table slot of subcarrier index k (0..N, DC at N / 2): FFT bin nn = lane + 64 m at [m / 4][lane][m % 4]"""
    nn = k - N // 2 if k >= N // 2 else k + 1024 - N // 2
    ln, m = nn & 63, nn >> 6
    return ((m >> 2) * 64 + ln) * 4 + (m & 3)


def _restate(psd):
    import dnrp
    sz = dnrp.compute_packet_sizes(dnrp.psdef(*psd))
    b, N_TS, N_eff, N_DF, N_SS, bps = psd[1], sz["N_TS"], sz["N_eff_TX"], sz["N_DF_symb"], sz["N_SS"], sz["N_bps"]
    txdiv = N_TS > 1 and N_SS == 1
    N = 56 * b
    cells = dnrp.query_table("symbol_cells", b, N_TS, N_eff, N_DF).astype(np.int64).reshape(-1, 3)
    pdc_off = np.concatenate([[0], np.cumsum(cells[:, 1])])
    pairs = dnrp.query_table("txdiv_pairs", N_TS).astype(np.int64).reshape(-1, 2) if N_TS > 1 else None
    kx, ky = (Q_BPSK_FX, Q_BPSK_FY) if bps == 1 else (1 << (bps - 1), 1 << (bps - 2))
    T = np.zeros((N_TS, N_DF + 1, 1024, 4), np.int64)
    T[:, 1:] = (ZB, 8, 8, Q_ZERO)
    stf = dnrp.query_table("stf", b, N_eff).view(np.complex64)
    for k in np.nonzero(stf)[0]:
        T[:, 0, _slot(int(k), N), 0] = 4  # CODE_STF
    # DRS: stream t's cells carry +-1 for the antenna of that stream alone
    drs = dnrp.query_table("drs_cells", b, N_TS, N_DF).astype(np.int64)
    nd, p = N // 4, 0
    while p < len(drs):
        l, t0, t1 = drs[p:p + 3]
        p += 3
        for t in range(t0, t1 + 1):
            val = dnrp.query_table("drs_values", b, t)
            for i in range(nd):
                T[t, l, _slot(int(drs[p + i]), N)] = (ZB, 8, 8, Q_DRS + (1 if val[i] < 0 else 0))
            p += nd

    def partner(ts, j):  # (symbol index, which sign is flipped: 0 none, 1 re, 2 im) or None
        A, B = pairs[(j >> 1) % len(pairs)]
        if ts == A:
            return j, 0
        if ts == B:
            return j ^ 1, 2 if j & 1 else 1
        return None

    pdc = dnrp.query_table("pdc_cells", b, N_TS, N_eff, N_DF).astype(np.int64).reshape(-1, 2)
    pcc = dnrp.pcc_cells(b, N_TS)
    for ts in range(N_TS):
        for j, (l, k) in enumerate(pdc):
            if txdiv:
                pr = partner(ts, j)
                if pr is None:
                    continue
                js, K = pr[0], (0, kx, ky)[pr[1]]
            else:
                js, K = j * N_SS + ts, 0
            ab = (((int(pdc_off[l]) & ~1) * N_SS * bps) >> 3) & ~15
            bit = js * bps - 8 * ab
            T[ts, l, _slot(int(k), N)] = (bit >> 3, 16 - (bit & 7) - bps, bps, K)
        for j, (l, k) in enumerate(pcc):  # the PCC is SFBC-paired in every mode
            pr = partner(ts, j)
            if pr is None:
                continue
            jp = pr[0]
            T[ts, l, _slot(int(k), N)] = (PCB + ((2 * jp) >> 3), 14 - ((2 * jp) & 7), 2, Q_QPSK ^ (0, 2, 1)[pr[1]])
    return T, (b, N_TS, N_eff, N_DF, N_SS, bps, int(txdiv))


@pytest.mark.parametrize("name", sorted(E.CODE_CASES))
def test_tx_code_oh(name):
    import dnrp
    psd = E.CODE_CASES[name]
    sz = dnrp.compute_packet_sizes(dnrp.psdef(*psd))
    if sz["N_TS"] == 1:  # one stream: no one-hot table (the kernel's TXS_SISO form reads the cell codes)
        args = (psd[1], 1, sz["N_eff_TX"], sz["N_DF_symb"], 1, sz["N_bps"], 0)
        assert len(dnrp.query_table("tx_code_oh", *args)) == 0
        return
    want, args = _restate(psd)
    got = dnrp.query_table("tx_code_oh", *args).astype(np.int64).reshape(want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (name, len(bad), bad[:4].tolist(), [(got[tuple(x)].tolist(), want[tuple(x)].tolist()) for x in bad[:4]])
    # what the kernel relies on: both bytes of a field inside the staging window (1 KiB, spatial multiplexing
    # 4 KiB) or the PCC bytes, the field inside the pair, a slot index inside the table
    df = got[:, 1:]
    is_pdc = (df[..., 0] < PCB)
    win = 1024 if args[6] else 4096
    assert (df[..., 0][is_pdc] + 1 < win).all() and (df[..., 0][~is_pdc] + 1 < PCB + 32).all()
    assert (df[..., 1] + df[..., 2] <= 16).all() and (df[..., 2] >= 1).all()
    assert (df[..., 3] < 268).all() and (df[..., 3][is_pdc] < 268).all()
    # 256-QAM symbols without PCC cells are read as one byte: the field is the pair's first byte
    if sz["N_bps"] == 8:
        assert ((df[..., 1] == 8) & (df[..., 2] == 8))[is_pdc | (df[..., 0] == ZB)].all()
    # every cell type occurs for every stream: PDC (its own symbols, or as the second stream of a pair the
    # flipped partners), PCC, DRS of both signs, empty
    for ts in range(sz["N_TS"]):
        ks = set(np.unique(df[ts][..., 3]).tolist())
        assert {Q_DRS, Q_DRS + 1, Q_ZERO} <= ks, (name, ts, sorted(ks))
        assert any(k < 256 or k >= Q_BPSK_FX for k in ks), (name, ts, sorted(ks))
        assert ks & {Q_QPSK, Q_QPSK ^ 1, Q_QPSK ^ 2}, (name, ts, sorted(ks))


def test_tx_code_oh_arguments():
    import dnrp
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("tx_code_oh", 16, 2, 2, 2, 1, 8)      # six arguments
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("tx_code_oh", 16, 2, 2, 2, 1, 9, 1)   # N_bps 9
