"""Inputs shared by tests/test_rx_grid_host.py and tests/test_gpu_rx_grid.py (TEST INFRASTRUCTURE): the
kernel instantiations that the RX launchers choose from (N_RX, N_eff_TX, N_bps) -- launch_rx_epoch,
launch_rx_fused, launch_rx_cells, launch_rx_cells_sm -- one table of cases that reaches those no other
parity table reaches, and the window recipe of tests/test_gpu_parity.py (rx_windows; that file's
_rx_windows is this function).

A packet with fewer transmit streams than the context has antennas gives the (4, 1), (4, 2), (8, 1),
(8, 2) pairs. The epoch, fused and wave-front-end cases use the smallest contexts with N_b_DFT_os = 1024
at 10/9, os_min 1: (u_max, 16, N_RX, 1, 10, 9) with u_max <= 2, and the packet at (u_max, 16) with the
shortest valid PacketLength of its N_eff_TX (subslots: one for N_eff_TX <= 2, three for 4). The
rx_cells_kernel cases that need no 1024-point geometry use the smallest b at which the packet is valid.
"""
import numpy as np

import oracle_py as O
import phy_fixtures as F

SEED = 11      # tests/test_gpu_parity.py _rx_parity
SEED_SM = 17   # ... test_rx_sm_mmse_parity


def tx_inputs(rng, n, sz):
    pcc = np.stack([O.pack_bits(F.random_bits(rng, 196)) for _ in range(n)])
    pdc = np.stack([O.pack_bits(F.random_bits(rng, sz["G"])) for _ in range(n)])
    assert pcc.shape == (n, 25) and pdc.shape == (n, (sz["G"] + 7) // 8)
    return pcc, pdc


def rx_windows(rng, ops, ocf, n_rx, snrs, cb=0):
    """Oracle-TX packets through a random N_RX x N_TX mixing, CFO and AWGN at per-packet SNRs.
    Returns the windows, sync reports (with a small residual CFO error), network IDs, PLCF types
    and the transmitted packed bits. No GPU: sizes from the oracle."""
    import dnrp
    sz = O.packet_sizes(ops)
    d = O.dims(ocf, ops)
    S, N_dft = d["N_packet_os_rs"], d["N_b_DFT_os"]
    n = len(snrs)
    pcc, pdc = tx_inputs(rng, n, sz)
    windows, reports, nids, types = [], [], [], []
    L, M = int(ocf[3]), int(ocf[4])
    for i in range(n):
        nid, pt = 100 + (i % 6), 1 + i % 2
        iq_tx, _ = O.tx(ocf, ops, pcc[i], pdc[i], S, codebook=cb, network_id=nid, plcf_type=pt)
        off = int(rng.integers(0, 32))
        cfo_dect = rng.uniform(-1.75, 1.75) * 2 * np.pi / N_dft  # rad per DECT sample
        win = F.channel(rng, iq_tx, n_rx, S, off, cfo_dect * M / L, snrs[i])
        windows.append(win)
        est = -cfo_dect + rng.uniform(-0.02, 0.02) * 2 * np.pi / N_dft
        reports.append(dnrp.SyncReport(off, float(est), 0.0, int(ops[0]), int(ops[1]), sz["N_eff_TX"]))
        nids.append(nid)
        types.append(pt)
    return windows, reports, nids, types, pcc, pdc


# Receivers a case runs through (tests/test_gpu_rx_grid.py): the environment, and the kernel whose launch
# count proves the receiver. "epoch": DNRP_RX_EPOCH=2 below 4 RX antennas, unset with 4 (the default path);
# "fused": DNRP_RX_FUSED=1; "ypath": DNRP_RX_EPOCH=0 (front end into Y, rx_cells_kernel<R, T, false, NBPS>);
# "sm": set_rx_mode(SM_MMSE) (rx_cells_kernel<R, T, true, NBPS>)
RECEIVERS = ("epoch", "fused", "ypath", "sm")

# name: (psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_RX, os_min, L, M), SNRs, receivers)
CASES = {
    # ---- N_b_DFT_os = 1024 at 10/9: epoch, fused, and the Y path's wave front end
    "r11_256": ((1, 16, 0, 1, 0, 8), (1, 16, 1, 1, 10, 9), (18.0, 32.0), ("epoch", "fused")),
    "r11_bpsk": ((1, 16, 0, 1, 0, 0), (1, 16, 1, 1, 10, 9), (3.0, 20.0), ("epoch",)),
    "r21_256": ((1, 16, 0, 1, 0, 8), (1, 16, 2, 1, 10, 9), (18.0, 32.0), ("epoch", "fused")),
    "r21_qpsk": ((2, 16, 0, 1, 0, 1), (2, 16, 2, 1, 10, 9), (5.0, 20.0), ("epoch", "fused")),
    "r41_256": ((2, 16, 0, 1, 0, 8), (2, 16, 4, 1, 10, 9), (18.0, 32.0), ("epoch", "fused")),
    "r41_16qam": ((1, 16, 0, 1, 0, 3), (1, 16, 4, 1, 10, 9), (8.0, 22.0), ("epoch",)),
    "r22_256": ((2, 16, 0, 1, 1, 8), (2, 16, 2, 1, 10, 9), (18.0, 34.0), ("epoch", "fused")),
    "r22_64qam": ((1, 16, 0, 1, 1, 5), (1, 16, 2, 1, 10, 9), (15.0, 28.0), ("epoch",)),
    "r42_256": ((1, 16, 0, 1, 1, 8), (1, 16, 4, 1, 10, 9), (18.0, 32.0), ("epoch", "fused")),
    "r42_qpsk": ((2, 16, 0, 1, 1, 2), (2, 16, 4, 1, 10, 9), (5.0, 20.0), ("epoch", "fused")),
    "r44_256": ((1, 16, 0, 3, 5, 8), (1, 16, 4, 1, 10, 9), (18.0, 34.0), ("epoch", "fused")),
    "r44_64qam": ((2, 16, 0, 3, 5, 7), (2, 16, 4, 1, 10, 9), (15.0, 28.0), ("epoch",)),
    # 8 RX antennas: (2, 16, 8, 1, 10, 9); no epoch instantiation, so the default path is the Y path
    "r81_256": ((2, 16, 0, 1, 0, 8), (2, 16, 8, 1, 10, 9), (18.0, 30.0), ("fused", "ypath")),
    "r81_16qam": ((2, 16, 0, 1, 0, 4), (2, 16, 8, 1, 10, 9), (8.0, 22.0), ("ypath",)),
    "r82_256": ((2, 16, 0, 1, 1, 8), (2, 16, 8, 1, 10, 9), (18.0, 32.0), ("fused", "ypath")),
    "r82_64qam": ((2, 16, 0, 1, 1, 6), (2, 16, 8, 1, 10, 9), (15.0, 28.0), ("ypath",)),
    "r84_256": ((2, 16, 0, 3, 5, 8), (2, 16, 8, 1, 10, 9), (32.0,), ("fused",)),
    # ---- rx_cells_kernel<R, T, false, NBPS> at the smallest b
    "y21_256": ((1, 1, 0, 1, 0, 8), (1, 1, 2, 1, 10, 9), (18.0, 32.0), ("ypath",)),
    "y41_256": ((1, 1, 0, 1, 0, 8), (1, 1, 4, 1, 10, 9), (18.0, 32.0), ("ypath",)),
    "y22_256": ((1, 1, 0, 1, 1, 8), (1, 1, 2, 1, 10, 9), (18.0, 34.0), ("ypath",)),
    "y42_256": ((1, 1, 0, 1, 1, 8), (1, 1, 4, 1, 10, 9), (18.0, 32.0), ("ypath",)),
    "y42_16qam": ((1, 1, 0, 1, 1, 3), (1, 1, 4, 1, 10, 9), (8.0, 22.0), ("ypath",)),
    "y84_64qam": ((1, 1, 0, 3, 5, 5), (1, 1, 8, 1, 10, 9), (15.0, 28.0), ("ypath",)),
    # ---- spatial multiplexing, rx_cells_kernel<R, T, true, NBPS>, at the smallest b
    "sm42_16qam": ((1, 1, 0, 1, 2, 3), (1, 1, 4, 1, 10, 9), (25.0, 32.0), ("sm",)),
    "sm42_64qam": ((1, 1, 0, 1, 2, 5), (1, 1, 4, 1, 10, 9), (30.0,), ("sm",)),
    "sm42_256": ((1, 1, 0, 1, 2, 8), (1, 1, 4, 1, 10, 9), (40.0,), ("sm",)),
    "sm22_256": ((1, 1, 0, 1, 2, 8), (1, 1, 2, 1, 10, 9), (40.0,), ("sm",)),
    "sm82_qpsk": ((1, 1, 0, 1, 2, 1), (1, 1, 8, 1, 10, 9), (15.0, 30.0), ("sm",)),
    "sm82_256": ((1, 1, 0, 1, 2, 8), (1, 1, 8, 1, 10, 9), (40.0,), ("sm",)),
    "sm84_64qam": ((1, 1, 0, 3, 6, 6), (1, 1, 8, 1, 10, 9), (30.0,), ("sm",)),
    "sm84_256": ((1, 1, 0, 3, 6, 8), (1, 1, 8, 1, 10, 9), (40.0,), ("sm",)),
}
NAMES = list(CASES)
RUNS = [(name, rcv) for name in NAMES for rcv in CASES[name][3]]

# One new class of each of epoch, fused and cells in chestim l mode, and one with stride 3:
# (case, receiver, chestim lr, stride)
VARIANTS = [
    ("r42_qpsk", "epoch", 0, 2), ("r44_64qam", "epoch", 1, 3),
    ("r82_256", "fused", 0, 2), ("r41_256", "fused", 1, 3),
    ("r81_16qam", "ypath", 0, 2), ("r82_64qam", "ypath", 1, 3),
]


def env_of(name, receiver):
    """the switches of a run: DNRP_RX_EPOCH unset with 4 RX antennas (the default takes the epoch receiver)"""
    n_rx = CASES[name][1][2]
    return {"epoch": {} if n_rx >= 4 else {"DNRP_RX_EPOCH": "2"}, "fused": {"DNRP_RX_FUSED": "1"},
            "ypath": {"DNRP_RX_EPOCH": "0"}, "sm": {}}[receiver]


def oracle_cfg(name, lr=1, stride=2):
    u_max, b_max, _, os_min, L, M = CASES[name][1]
    return O.cfg(u_max, b_max, os_min, L, M, lr=lr, stride=stride)


def is_sm(name):
    return CASES[name][3] == ("sm",)


SYNC_RMS_0 = 0.123  # packet 0's sync report carries an RMS for antenna 0 only (tests/test_gpu_parity.py)

_WIN = {}


def windows(name):
    """(windows, reports, nids, types, pdc, sync_rms) of a case: a pure function of the case, computed once.
    Outside spatial multiplexing packet 0's sync report carries SYNC_RMS_0 for antenna 0, as in _rx_parity."""
    if name not in _WIN:
        psd, ctx, snrs, _ = CASES[name]
        sm = is_sm(name)
        rng = np.random.default_rng(SEED_SM if sm else SEED)
        w, reports, nids, types, _, pdc = rx_windows(rng, O.psdef(*psd), oracle_cfg(name), ctx[2], snrs)
        sync_rms = [None] * len(w)
        if not sm:
            reports[0].rms[0] = SYNC_RMS_0
            sync_rms[0] = [SYNC_RMS_0] + [0.0] * 7
        for x in w:
            x.setflags(write=False)
        _WIN[name] = (w, reports, nids, types, pdc, sync_rms)
    return _WIN[name]


_REF = {}


def oracle(name, i, lr=1, stride=2, use_float=False):
    """the oracle's RX of packet i of a case (its double path unless use_float), computed once"""
    key = (name, i, lr, stride, use_float)
    if key not in _REF:
        w, reports, nids, types, _, sync_rms = windows(name)
        _REF[key] = O.rx(oracle_cfg(name, lr, stride), O.psdef(*CASES[name][0]), w[i], reports[i].fine_peak_time,
                         float(np.float32(reports[i].cfo_fractional_rad)), nids[i], types[i], use_float=use_float,
                         sync_rms=sync_rms[i], sm_mmse=is_sm(name))
    return _REF[key]


def nbps_class(n_bps, sm):
    """the demapper width compiled into the instantiation: 8 (and 6 with spatial multiplexing), else 0"""
    return n_bps if n_bps == 8 or (sm and n_bps == 6) else 0


def wave_geometry(psd, ctx):
    """N_b_DFT_os = 1024 with the compiled-in 9/10 resampler: the epoch and fused receivers' geometry, and
    the Y path's wave front end"""
    u_max, b_max, _, os_min, L, M = ctx
    return (os_min, L, M) == (1, 10, 9) and O.dims(O.cfg(u_max, b_max, os_min, L, M), O.psdef(*psd))["N_b_DFT_os"] == 1024
