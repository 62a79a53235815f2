"""Inputs of tests/test_gpu_tx_stream_edges.py and tests/test_tx_stream_codes_host.py (TEST INFRASTRUCTURE): the
edges of the streaming TX kernel (kernels/tx.hip tx_stream_kernel) around its PDC byte staging and its one-hot
code table. Every packet is the shortest of its mode that launch_tx sends to the streaming family
(N_b_DFT_os = 1024 at 10/9 with a 9-pattern STF: u = 2, b = 16); tests/tx_grid_cases.py names the forms.

The PDC rows of a case: three rows at the case's byte stride in one allocation of exactly
2 * stride + ceil(G / 8) bytes, so the last packet's last byte is the allocation's last. Rows 0 and 2 hold
random bits, row 1 holds 0xFF in every byte (a packet of ones), and so do the bytes between a row's end and
the next row. A load past a row's end therefore reads ones (or the next packet), a load that stops short of
it drops bits of the packet's last cells.
"""
import numpy as np

import oracle_py as O
import tx_grid_cases as G

N_ROWS = 3

# name: (psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_TX_max, os_min, L, M), codebook,
#        bytes of a row past ceil(G / 8): 0 = rows back to back, the fields of the form the case is there for)
CASES = {
    # ---- the one-hot forms, 256-QAM (one byte per symbol) and 64-QAM (bit fields), rows back to back and at
    # a stride that is no multiple of 16
    "txdiv1_256_b2b": ((2, 16, 0, 1, 1, 8), (2, 16, 2, 1, 10, 9), 0, 0, dict(mode=G.TXS_TXDIV1, q8=1, n_seg=1)),
    "txdiv1_256_pad": ((2, 16, 0, 1, 1, 8), (2, 16, 2, 1, 10, 9), 0, 5, dict(mode=G.TXS_TXDIV1, q8=1, n_seg=1)),
    "txdiv1_64_b2b": ((2, 16, 0, 1, 1, 5), (2, 16, 2, 1, 10, 9), 0, 0, dict(mode=G.TXS_TXDIV1, q8=0, n_seg=1)),
    "txdiv1_64_pad": ((2, 16, 0, 1, 1, 5), (2, 16, 2, 1, 10, 9), 0, 3, dict(mode=G.TXS_TXDIV1, q8=0, n_seg=1)),
    # BPSK: one index bit for both signs, the SFBC partner's flipped points are table slots of their own
    "txdiv1_bpsk_pad": ((2, 16, 0, 1, 1, 0), (2, 16, 2, 1, 10, 9), 0, 7, dict(mode=G.TXS_TXDIV1, q8=0, n_seg=1)),
    # four transmit streams: every pair of the SFBC schedule, the DRS symbol ahead of the PCC symbol
    "txdiv1_4ts_256_b2b": ((2, 16, 0, 3, 5, 8), (2, 16, 4, 1, 10, 9), 0, 0, dict(mode=G.TXS_TXDIV1, q8=1, n_seg=1)),
    # ---- the other modes, one case each
    "sm1_256_pad": ((2, 16, 0, 1, 2, 8), (2, 16, 2, 1, 10, 9), 0, 9, dict(mode=G.TXS_SM1, q8=1, n_seg=1, sb_chunks=2)),
    "siso_16qam_pad": ((2, 16, 0, 1, 0, 3), (2, 16, 1, 1, 10, 9), 0, 2, dict(mode=G.TXS_SISO, q8=0, n_seg=1)),
    "txdiv_16qam_b2b": ((2, 16, 0, 1, 1, 3), (2, 16, 2, 1, 10, 9), 1, 0, dict(mode=G.TXS_TXDIV, q8=0, n_seg=1)),
    # ---- a batch small enough for two segments per packet: the second starts with a history piece
    "txdiv1_256_seg2": ((2, 16, 0, 4, 1, 8), (2, 16, 2, 1, 10, 9), 0, 11, dict(mode=G.TXS_TXDIV1, q8=1, n_seg=2)),
}
NAMES = list(CASES)
# run once with dnrp_ctx_set_tx_windowing(G.FRACTION) against the numpy reference of tests/test_gpu_tx_window.py
WINDOWED = "txdiv1_256_pad"

# the code table's host cases: a subslot and a full-slot packet at b = 16, N_TS = 1, 2, 4 (tm 0, 1, 5),
# 256-QAM, 64-QAM and BPSK, and spatial multiplexing (tm 2)
CODE_CASES = {
    "sub_ts1": (2, 16, 0, 1, 0, 8),
    "sub_ts2_256": (2, 16, 0, 1, 1, 8),
    "sub_ts2_64": (2, 16, 0, 1, 1, 5),
    "sub_ts2_bpsk": (2, 16, 0, 1, 1, 0),
    "sub_ts4_256": (2, 16, 0, 3, 5, 8),
    "slot_ts1": (2, 16, 1, 1, 0, 8),
    "slot_ts2_256": (2, 16, 1, 1, 1, 8),
    "slot_ts4_64": (2, 16, 1, 1, 5, 6),
    "sub_sm2_256": (2, 16, 0, 1, 2, 8),
    "sub_sm2_16": (2, 16, 0, 1, 2, 3),
}


def rows(name, sz):
    """(pcc [3, 25], pdc bytes [3, ceil(G / 8)], the flat PDC allocation, its stride) of a case"""
    extra = CASES[name][3]
    nb = (sz["G"] + 7) // 8
    stride = nb + extra
    rng = np.random.default_rng(0xED6E5)
    pcc = np.stack([O.pack_bits(rng.integers(0, 2, 196, dtype=np.uint8)) for _ in range(N_ROWS)])
    pdc = np.stack([O.pack_bits(rng.integers(0, 2, sz["G"], dtype=np.uint8)) for _ in range(N_ROWS)])
    pdc[1, :] = 0xFF
    flat = np.full((N_ROWS - 1) * stride + nb, 0xFF, np.uint8)
    for i in range(N_ROWS):
        flat[i * stride: i * stride + nb] = pdc[i]
    return pcc, pdc, flat, stride
