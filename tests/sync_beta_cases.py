"""Inputs shared by tests/test_sync_beta_host.py and tests/test_gpu_sync_beta.py (TEST INFRASTRUCTURE):
oracle-TX packets of bandwidth b in the window of a receiver of class (u, b_max, os_min, L, M), and the
beta estimator of coarse_peak_f_domain_t::estimate_beta restated in numpy (double).

Every window: 30 dB, MCS 1, one random N_RX x N_TX mixing per packet, a CFO within +-1.75 subcarriers of
the class rate, the packet start at least two STFs into the window. The windows are a pure function of
their case (seeded), so both files see the same samples.
"""
import zlib

import numpy as np

import oracle_py as O
import phy_fixtures as F

B_IDX2B = (1, 2, 4, 8, 12, 16)
SNR_DB = 30.0

# (u, b_max, os_min, L, M, n_ant, tm, b)
# L = M = 1, b_max / b an integer: the oracle search of (u, b, os_min b_max / b) is the reference
PARITY = [(1, 4, 1, 1, 1, 1, 0, 1), (1, 4, 1, 1, 1, 1, 0, 2), (1, 4, 1, 1, 1, 1, 0, 4),
          (1, 4, 1, 1, 1, 2, 1, 1), (1, 4, 1, 1, 1, 2, 1, 2),
          (2, 8, 1, 1, 1, 4, 5, 1), (2, 8, 1, 1, 1, 4, 5, 4), (2, 8, 1, 1, 1, 4, 5, 8),
          (1, 2, 2, 1, 1, 2, 1, 1)]
# no oracle search with these filters / ratios: checked against the transmitted truth
TRUTH = [(1, 4, 1, 10, 9, 2, 1, 1), (1, 4, 1, 10, 9, 2, 1, 2), (2, 8, 1, 10, 9, 4, 5, 2),
         (1, 12, 1, 40, 27, 1, 0, 8), (1, 12, 1, 1, 1, 1, 0, 8), (1, 12, 1, 1, 1, 1, 0, 12),
         # os_min 2 at 10/9: sync_beta_kernel<9, 10, 4>
         (1, 2, 2, 10, 9, 2, 1, 1), (1, 2, 2, 10, 9, 2, 1, 2)]
N_WINDOWS = 2


def case_id(c):
    return "u%d_bmax%d_os%d_%d_%d_ant%d_tm%d_b%d" % c


def psdef(c):
    u, _, _, _, _, _, tm, b = c
    return (u, b, 1, 1, tm, 1)


def geometry(c):
    """Sizes of a case: the packet's slot length and STF length in hw samples, N of the class rate."""
    u, b_max, os_min, L, M, _, _, _ = c
    cf = O.cfg(u, b_max, os_min=os_min, L=L, M=M)
    S = O.dims(cf, O.psdef(*psdef(c)))["N_packet_os_rs"]
    N = 64 * b_max * os_min
    stf_hw = (N + N // 4 * (3 if u == 1 else 5)) * L // M
    return dict(S=S, N=N, stf_hw=stf_hw, S_win=2 * stf_hw + 32 + S + stf_hw)


def packet(rng, c, cfo_dect_rad, i=0):
    """One oracle-TX packet of the case, mixed onto the case's antennas: (y [n_ant, S], meta)."""
    u, b_max, os_min, L, M, n_ant, _, _ = c
    cf, ps = O.cfg(u, b_max, os_min=os_min, L=L, M=M), O.psdef(*psdef(c))
    sz = O.packet_sizes(ps)
    S = O.dims(cf, ps)["N_packet_os_rs"]
    pcc = rng.integers(0, 256, 25, dtype=np.uint8)
    pdc = rng.integers(0, 256, (sz["G"] + 7) // 8, dtype=np.uint8)
    nid, pt = 100 + i % 6, 1 + i % 2
    x, _ = O.tx(cf, ps, pcc, pdc, S, network_id=nid, plcf_type=pt, phase_inc=cfo_dect_rad * M / L)
    return F.mixing_matrix(rng, n_ant, x.shape[0]) @ x, (pcc, pdc, nid, pt)


def add_noise(rng, win, p_sig):
    sigma = np.sqrt(p_sig / 10 ** (SNR_DB / 10) / 2)
    return (win + sigma * (rng.standard_normal(win.shape) + 1j * rng.standard_normal(win.shape))).astype(np.complex64)


def draw_cfo(rng, c):
    return rng.uniform(-1.75, 1.75) * 2 * np.pi / (64 * c[1] * c[2])


_CACHE = {}


def windows(c):
    """The N_WINDOWS windows of a case: list of (window complex64 [n_ant, S_win], start, meta, cfo)."""
    if c not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
        g = geometry(c)
        out = []
        for i in range(N_WINDOWS):
            start, cfo = 2 * g["stf_hw"] + int(rng.integers(0, 32)), draw_cfo(rng, c)
            y, meta = packet(rng, c, cfo, i)
            win = np.zeros((c[5], g["S_win"]), np.complex128)
            win[:, start:start + g["S"]] = y
            out.append((add_noise(rng, win, np.mean(np.abs(y[:, : g["S"] // 2]) ** 2)), start, meta, cfo))
        _CACHE[c] = out
    return _CACHE[c]


# two packets of different b in one window (seed 77) and in a ring (seed 78)
MIXED_WINDOW = ((1, 4, 1, 1, 1, 1, 0, 1), (1, 4, 1, 1, 1, 1, 0, 4))
MIXED_RING = ((1, 4, 1, 1, 1, 1, 0, 2), (1, 4, 1, 1, 1, 1, 0, 1))


def two_packet_window(seed, c_first, c_second):
    """one window of the shared class holding a packet of each case: (window, [start, start])"""
    rng = np.random.default_rng(seed)
    g = geometry(c_first)
    starts = [2 * g["stf_hw"] + 11, 2 * g["stf_hw"] + 11 + g["S"] + 3 * g["stf_hw"] + 5]
    win = np.zeros((c_first[5], starts[1] + g["S"] + g["stf_hw"]), np.complex128)
    p = []
    for i, (c, st) in enumerate(zip((c_first, c_second), starts)):
        y, _ = packet(rng, c, draw_cfo(rng, c), i)
        win[:, st:st + g["S"]] += y
        p.append(np.mean(np.abs(y[:, : g["S"] // 2]) ** 2))
    return add_noise(rng, win, np.mean(p)), starts


def chunk_len(c):
    return geometry(c)["S_win"] * 7 // 8


def oracle_sync_cfg(c):
    """The oracle search a b packet in the (b_max, os_min) stream at L = M = 1 is exactly: the class of b at
    os_min b_max / b has the same bos, the same geometry and the template of b."""
    u, b_max, os_min, L, M, n_ant, _, b = c
    assert L == M == 1 and b_max % b == 0
    return O.sync_cfg(u, b, os_min=os_min * b_max // b, L=1, M=1, n_ant=n_ant, chunk_len=chunk_len(c))


def band_ratios(x, u, b_max, os_min, at):
    """estimate_beta's inputs in double: x [n_ant, S] DECT-rate samples, `at` the coarse peak. Returns the
    list of (b_tested, ratio) of every widening step up to b_max, whatever the threshold."""
    N = 64 * b_max * os_min
    cp = N // 4 * (3 if u == 1 else 5)
    seg = np.zeros((x.shape[0], N), np.complex128)
    have = x[:, at + cp: at + cp + N]
    seg[:, : have.shape[1]] = have
    P = (np.abs(np.fft.fftshift(np.fft.fft(seg, axis=1), axes=1)) ** 2).sum(0)
    lo, hi, b_est, centre, out = N // 2 - 32, N // 2 + 32, 1, None, []
    centre = P[lo:hi].sum()
    for bt in B_IDX2B[1:]:
        if bt > b_max:
            break
        n = (bt - b_est) * 32
        side = P[lo - n:lo].sum() + P[hi:hi + n].sum()
        out.append((bt, (side / (2 * n)) / (centre / (64 * b_est))))
        lo, hi, b_est, centre = lo - n, hi + n, bt, centre + side
    return out


def estimate_beta(x, u, b_max, os_min, at, threshold_linear):
    """(b_est, ratios formed): from b = 1 the next b while the ratio exceeds the threshold, ending at b_max."""
    b_est, formed = 1, []
    for bt, r in band_ratios(x, u, b_max, os_min, at):
        formed.append(r)
        if not r > threshold_linear:
            break
        b_est = bt
    return b_est, formed
