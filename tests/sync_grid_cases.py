"""Inputs shared by tests/test_sync_grid_host.py and tests/test_gpu_sync_grid.py (TEST INFRASTRUCTURE):
the sync geometry classes whose kernel forms are chosen by size inside a template instantiation
(kernels/sync_*.hip launch_*: step = 4 b os_min, pattern, stf_len, D, n_uw, log2_fft), one case per class,
and one window recipe for all of them.

Every window: MCS 1 unless the case says otherwise, one random N_RX x N_TX mixing, a CFO within +-1.75
subcarriers, 30 dB, the start in [stf_hw / 2, 3 stf_hw / 2). Three packet windows and one of noise only,
from default_rng(21). The windows are a pure function of their case, so both files see the same samples.
"""
import numpy as np

import oracle_py as O
import phy_fixtures as F

# name: (psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_TX_max, os_min, L, M))
CASES = {
    "u1b2": ((1, 2, 1, 1, 0, 1), (1, 2, 1, 1, 10, 9)),          # step 8, 512-point fine, n_uw 6
    "u1b4": ((1, 4, 1, 1, 0, 1), (1, 4, 1, 1, 10, 9)),          # step 16 on the hl-24 stream kernel
    "u2b12": ((2, 12, 1, 1, 0, 1), (2, 12, 1, 1, 10, 9)),       # step 48, sq 12
    "u1b12": ((1, 12, 1, 1, 0, 1), (1, 12, 1, 1, 10, 9)),       # step 48 with n_uw 6, 2048-point
    "u1b16": ((1, 16, 1, 1, 0, 1), (1, 16, 1, 1, 10, 9)),       # pipe kernel, 7 patterns
    "lm1_u1b2": ((1, 2, 1, 1, 0, 1), (1, 2, 1, 1, 1, 1)),       # <1, 1, 0>, 512-point, n_uw 6
    "os2_u1b12": ((1, 12, 1, 1, 0, 1), (1, 12, 1, 2, 10, 9)),   # <9, 10, 4> step 96, n_uw 6
    "os2_u2b12": ((2, 12, 1, 1, 0, 1), (2, 12, 1, 2, 10, 9)),   # 8192-point fine, split rounds allowed
    "os2_u2b16_tm1": ((2, 16, 1, 1, 1, 1), (2, 16, 2, 2, 10, 9)),  # step 128, sync_peak_ok false, 2 antennas
    "os2_C4": F.PARITY_CASES["os2_C4"][:2],                     # the same class with 4 antennas, 3 templates
    "lm40_u2b16": ((2, 16, 1, 1, 0, 1), (2, 16, 1, 1, 40, 27)),  # <0, 0, 0> with 8192-point fine
}
NAMES = list(CASES)
N_PACKET_WINDOWS = 3
MAX_REPORTS = 2
SNR_DB = 30.0
SEED = 21

# dnrp_rx_sync_batch declines the class (2, 16) of this context (a 16384-point fine search); the class
# (2, 2) of the same context is searched after the refusal, on windows of UNSUPPORTED_FOLLOWUP
UNSUPPORTED_CTX = (2, 16, 1, 2, 40, 27)
UNSUPPORTED_SYNC = (2, 16)
UNSUPPORTED_FOLLOWUP = ((2, 2, 1, 1, 0, 1), (2, 2, 1, 2, 40, 27))


def case_def(case):
    """a name of CASES or a (psdef, ctx) pair"""
    return CASES[case] if isinstance(case, str) else case


def lr(name):
    return F.PARITY_CASES[name][2] if name in F.PARITY_CASES else 1


def oracle_sync_cfg(name, chunk_len=0):
    psd, (_, _, n_ant, os_min, L, M) = case_def(name)
    return O.sync_cfg(psd[0], psd[1], os_min=os_min, L=L, M=M, n_ant=n_ant, chunk_len=chunk_len)


def sync_geometry(name):
    return O.sync_geometry(oracle_sync_cfg(name))


def log2_fft(g):
    """smallest power of two >= xc_len - 1 + tmpl_len"""
    lg = 0
    while (1 << lg) < g["xc_len"] - 1 + g["tmpl_len"]:
        lg += 1
    return lg


def recipe(name):
    """(stf_hw, chunk_len, S_win) of a case"""
    psd, (_, _, _, os_min, L, M) = case_def(name)
    n_pattern = 7 if psd[0] == 1 else 9
    stf_hw = 16 * n_pattern * psd[1] * os_min * L // M
    chunk_len = 2 * stf_hw
    return stf_hw, chunk_len, (chunk_len + 8 * stf_hw + 512 + 1) & ~1


def sync_window(rng, name, S_win, starts, cfo_dect_rad, snr_db=SNR_DB):
    """phy_fixtures.sync_window for a case of this file (the same draws in the same order): one window
    complex64 [n_ant, S_win] of oracle-TX packets at the hw-sample offsets `starts`. Returns
    (window, [(pcc_d, pdc_d, network_id, plcf_type)])."""
    psd, cfgt = case_def(name)
    cf = O.cfg(cfgt[0], cfgt[1], os_min=cfgt[3], L=cfgt[4], M=cfgt[5])
    ps = O.psdef(*psd)
    sz = O.packet_sizes(ps)
    n_rx = cfgt[2]
    S_slot = O.dims(cf, ps)["N_packet_os_rs"]
    win = np.zeros((n_rx, S_win), np.complex128)
    meta, p_sig = [], []
    for i, st in enumerate(starts):
        pcc = rng.integers(0, 256, 25, dtype=np.uint8)
        pdc = rng.integers(0, 256, (sz["G"] + 7) // 8, dtype=np.uint8)
        nid, pt = 100 + i % 6, 1 + i % 2
        x, _ = O.tx(cf, ps, pcc, pdc, S_slot, network_id=nid, plcf_type=pt, phase_inc=cfo_dect_rad * cfgt[5] / cfgt[4])
        y = F.mixing_matrix(rng, n_rx, x.shape[0]) @ x
        n = min(S_slot, S_win - st)
        win[:, st:st + n] += y[:, :n]
        p_sig.append(np.mean(np.abs(y[:, : S_slot // 2]) ** 2))
        meta.append((pcc, pdc, nid, pt))
    p = np.mean(p_sig) if p_sig else 0.05
    sigma = np.sqrt(p / 10 ** (snr_db / 10) / 2)
    win += sigma * (rng.standard_normal(win.shape) + 1j * rng.standard_normal(win.shape))
    return win.astype(np.complex64), meta


def draw_cfo(rng, name):
    psd, cfgt = case_def(name)
    return rng.uniform(-1.75, 1.75) * 2 * np.pi / (64 * psd[1] * cfgt[3])


_CACHE = {}


def windows(name):
    """(windows, starts): N_PACKET_WINDOWS windows of one packet each, then one of noise only; starts
    holds the transmitted start of every packet window."""
    if name not in _CACHE:
        rng = np.random.default_rng(SEED)
        stf_hw, _, S_win = recipe(name)
        wins, starts = [], []
        for _ in range(N_PACKET_WINDOWS):
            start = int(rng.integers(stf_hw // 2, 3 * stf_hw // 2))
            cfo = draw_cfo(rng, name)
            wins.append(sync_window(rng, name, S_win, [start], cfo)[0])
            starts.append(start)
        wins.append(sync_window(rng, name, S_win, [], 0.0)[0])
        _CACHE[name] = (wins, starts)
    return _CACHE[name]


_REFS = {}


def oracle_reports(name):
    """the oracle's reports (max_reports = MAX_REPORTS) of every window of the case, computed once"""
    if name not in _REFS:
        osc = oracle_sync_cfg(name, recipe(name)[1])
        _REFS[name] = [O.sync(osc, w, max_reports=MAX_REPORTS) for w in windows(name)[0]]
    return _REFS[name]
