"""RX windows through a frequency-selective, time-varying channel with a timing error in the sync report
(TEST INFRASTRUCTURE, no GPU needed): shared by tests/test_rx_selective_host.py (CPU: the inputs are fair,
do what they claim, and tell wrong receivers from the right one, from the oracle alone) and
tests/test_gpu_rx_selective.py (GPU parity on the same windows).

Every other RX parity table feeds the receiver phy_fixtures.channel: one complex matrix per packet, flat
over frequency, constant over the packet (exactly 1 for SISO), the packet start known to the sample. Here
each (rx, tx) link is a tapped delay line:

  y[r, n] = sum_t sum_p a[r, t, p] exp(2 pi j f[r, t, p] n / S) x[t, n - d_p]

 - delays d_p whole hw samples inside the cyclic prefix, the largest D = max(3, round(0.58 CP_hw / 2)) with
   CP_hw = CP_os L / M: 3 at N_b_DFT_os = 64, 41 at 1024 points at 10/9;
 - three taps (0, D / 3, D) at 0 / -6 / -10 dB for b <= 4, four taps (0, 0.17 D, 0.56 D, D) at
   0 / -5 / -9 / -13 dB above, normalised to unit power and divided by sqrt(N_TX);
 - an independent uniform phase per tap and link (1 x 1 links too), and an independent Doppler per tap and
   link, uniform in +-DOPPLER_CYCLES cycles over the packet;
 - the sync report's fine_peak_time is the true offset plus e: packet 0 early (e in {-3, -2}), packet 1
   late (e in {+1, +2}); CFO and its residual error as in rx_grid_cases.rx_windows;
 - AWGN relative to the power of the first half of the noiseless signal, the window truncated to
   N_samples_packet_os_rs (the guard interval absorbs the tails).
"""
import functools

import numpy as np

import oracle_py as O
import phy_fixtures as F
import rx_grid_cases as G

SEED = 4100
DOPPLER_CYCLES = 0.15
EARLY, LATE = (-3, -2), (1, 2)
PROFILE_3 = (0.0, -6.0, -10.0)
PROFILE_4 = (0.0, -5.0, -9.0, -13.0)
SYNC_RMS_0 = G.SYNC_RMS_0

# (case, receiver, chestim lr, stride). Cases named r*, y*, sm* are rows of rx_grid_cases.CASES (receivers
# as there), the others rows of phy_fixtures.PARITY_CASES on the path the context takes by default, with
# their own chestim mode and codebook.
RUNS = [
    # ---- the 1024-point wave geometry
    ("r11_256", "epoch", 1, 2), ("r11_256", "ypath", 1, 2),
    ("r22_256", "epoch", 1, 2), ("r22_256", "fused", 1, 2),
    ("r42_qpsk", "epoch", 0, 2),
    ("r41_16qam", "epoch", 1, 2),
    ("r44_256", "epoch", 1, 2),       # rx_epoch_kernel<4, 4, 8> on the default path
    ("r44_256", "fused", 1, 2),       # the one fused run whose packet holds lr stages (test_lr_mode_is_reached)
    ("r44_64qam", "epoch", 1, 3),
    ("r81_16qam", "ypath", 1, 2),
    ("r82_256", "fused", 1, 2),
    # ---- small b through rx_cells_kernel
    ("y21_256", "ypath", 1, 2), ("y42_16qam", "ypath", 1, 2), ("y84_64qam", "ypath", 1, 2),
    # ---- spatial multiplexing through the MMSE receiver
    ("sm42_16qam", "sm", 1, 2), ("sm84_64qam", "sm", 1, 2), ("sm22_256", "sm", 1, 2),
    # ---- other front ends and resamplers
    ("C2", "default", 1, 2), ("mrc2_64qam", "default", 1, 2), ("tm1_txdiv2", "default", 1, 2),
    ("tm5_u2b4", "default", 1, 2), ("tm3_codebook3", "default", 1, 2), ("lmode_siso", "default", 0, 2),
    ("lmode_txdiv2", "default", 0, 2), ("lm40_27_b12", "default", 1, 2), ("lm1_1_tm1", "default", 1, 2),
    ("os2_u2b2_tm1", "default", 1, 2),
]
NAMES = list(dict.fromkeys(r[0] for r in RUNS))

# per-packet SNRs (dB) where the source table's would not do: the second packet at 20 dB or more for the
# sanity bound, 256-QAM over a selective channel clear of the error floor
SNRS = {
    "C2": (10.0, 25.0),
    "lmode_siso": (10.0, 22.0),
    "lm1_1_tm1": (12.0, 25.0),
    "sm84_64qam": (25.0, 30.0),   # one packet in rx_grid_cases
    "sm22_256": (30.0, 40.0),
}
# seeds of rows whose first draw missed a condition of tests/test_rx_selective_host.py (docs/DESIGN_LOG.md)
SEEDS = {"r11_256": 4301, "C2": 4441, "mrc2_64qam": 4451, "lm1_1_tm1": 4523, "lmode_siso": 4493, "sm22_256": 4434}


def spec(name):
    """(psdef tuple, ctx tuple (u_max, b_max, N_RX, os_min, L, M), SNRs, codebook, sm) of a case"""
    if name in G.CASES:
        psd, ctx, snrs, _ = G.CASES[name]
        cb = 0
    else:
        psd, ctx, _, snrs, cb = F.PARITY_CASES[name]
    snrs = SNRS.get(name, snrs)
    assert len(snrs) == 2, name
    return psd, ctx, snrs, cb, name in G.CASES and G.is_sm(name)


def oracle_cfg(name, lr=1, stride=2):
    u_max, b_max, _, os_min, L, M = spec(name)[1]
    return O.cfg(u_max, b_max, os_min, L, M, lr=lr, stride=stride)


def tap_profile(name):
    """(delays in hw samples, gains in dB) of a case, from its FFT size and resampling ratio"""
    psd, ctx = spec(name)[:2]
    d = O.dims(oracle_cfg(name), O.psdef(*psd))
    cp_hw = d["CP_os"] * ctx[4] / ctx[5]
    D = max(3, int(round(0.58 * cp_hw / 2)))
    if psd[1] <= 4:
        return (0, max(1, int(round(D / 3))), D), PROFILE_3
    return (0, int(round(0.17 * D)), int(round(0.56 * D)), D), PROFILE_4


def selective_channel(rng, iq_tx, n_rx, S_in, offset, cfo_hw_rad, snr_db, delays, gains_db, doppler_cycles):
    """iq_tx complex64 [N_TX, S] -> (rx window complex64 [n_rx, S_in], taps): the tapped-delay sum of the
    module docstring in complex128, placed at `offset`, CFO, AWGN as phy_fixtures.channel measures it.
    taps: dict(a=[n_rx, N_TX, P] complex amplitudes at the packet start, f=[n_rx, N_TX, P] cycles over the
    packet, delays, S)."""
    n_tx, S = iq_tx.shape
    P = len(delays)
    g = 10.0 ** (np.asarray(gains_db, np.float64) / 20)
    g = g / np.sqrt(np.sum(g * g) * n_tx)
    a = g[None, None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (n_rx, n_tx, P)))
    f = rng.uniform(-doppler_cycles, doppler_cycles, (n_rx, n_tx, P))
    x = iq_tx.astype(np.complex128)
    t = np.arange(S) / S
    y = np.zeros((n_rx, S), np.complex128)
    for p, d in enumerate(delays):
        xd = np.zeros_like(x)
        xd[:, d:] = x[:, : S - d]
        for r in range(n_rx):
            y[r] += np.sum(a[r, :, p, None] * np.exp(2j * np.pi * f[r, :, p, None] * t[None, :]) * xd, axis=0)
    out = np.zeros((n_rx, S_in), np.complex128)
    n = min(S, S_in - offset)
    out[:, offset:offset + n] = y[:, :n]
    out *= np.exp(1j * cfo_hw_rad * np.arange(S_in))[None, :]
    if snr_db is not None:
        p_sig = np.mean(np.abs(y[:, : S // 2]) ** 2)
        sigma = np.sqrt(p_sig / 10 ** (snr_db / 10) / 2)
        out += sigma * (rng.standard_normal(out.shape) + 1j * rng.standard_normal(out.shape))
    return out.astype(np.complex64), dict(a=a, f=f, delays=tuple(delays), S=S)


def seed_of(name):
    return SEEDS.get(name, SEED + NAMES.index(name))


@functools.lru_cache(maxsize=None)
def windows(name):
    """The case's two packets, built once: a list of dicts with the window (complex64 [N_RX, S], read-only),
    the sync report's fields (fine peak = true offset + e, CFO estimate with a small residual error, RMS of
    antenna 0 for packet 0 outside spatial multiplexing), network ID, PLCF type, the transmitted packed
    bits, the SNR, the timing error and the taps."""
    psd, ctx, snrs, cb, sm = spec(name)
    n_rx, L, M = ctx[2], ctx[4], ctx[5]
    ocf, ops = oracle_cfg(name), O.psdef(*psd)
    sz = O.packet_sizes(ops)
    d = O.dims(ocf, ops)
    S, n_dft = d["N_packet_os_rs"], d["N_b_DFT_os"]
    delays, gains = tap_profile(name)
    rng = np.random.default_rng(seed_of(name))
    out = []
    for i, snr in enumerate(snrs):
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + (i % 6), 1 + i % 2
        iq_tx, _ = O.tx(ocf, ops, pcc, pdc, S, codebook=cb, network_id=nid, plcf_type=pt)
        off = int(rng.integers(3, 32))  # the early report stays inside the window
        e = int(rng.choice(EARLY if i == 0 else LATE))
        cfo_dect = rng.uniform(-1.75, 1.75) * 2 * np.pi / n_dft  # rad per DECT sample
        win, taps = selective_channel(rng, iq_tx, n_rx, S, off, cfo_dect * M / L, snr, delays, gains, DOPPLER_CYCLES)
        est = -cfo_dect + rng.uniform(-0.02, 0.02) * 2 * np.pi / n_dft
        win.setflags(write=False)
        out.append(dict(win=win, fine_peak=off + e, offset=off, e=e, cfo_est=float(np.float32(est)), nid=nid, pt=pt,
                        pcc=pcc, pdc=pdc, sync_rms=[SYNC_RMS_0] + [0.0] * 7 if i == 0 and not sm else None,
                        snr=snr, taps=taps))
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, i, lr=1, stride=2, use_float=False, mutate=0):
    """The oracle's RX of packet i of a case, computed once per argument set (read-only)."""
    psd, _, _, _, sm = spec(name)
    w = windows(name)[i]
    r = O.rx(oracle_cfg(name, lr, stride), O.psdef(*psd), w["win"], w["fine_peak"], w["cfo_est"], w["nid"], w["pt"],
             use_float=use_float, sync_rms=w["sync_rms"], sm_mmse=sm, mutate=mutate)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def link_response(name, i):
    """|H| [N_RX, N_TX, N_b_OCC] over the occupied subcarriers at the packet start, from packet i's taps"""
    psd, ctx = spec(name)[:2]
    ops = O.psdef(*psd)
    d = O.dims(oracle_cfg(name), ops)
    n_occ = O.packet_sizes(ops)["N_b_OCC"]
    k = np.concatenate([np.arange(-n_occ // 2, 0), np.arange(1, n_occ // 2 + 1)])
    taps = windows(name)[i]["taps"]
    # a delay of d hw samples is d M / L samples at the FFT's rate
    ph = np.exp(-2j * np.pi * k[None, :] * (np.asarray(taps["delays"])[:, None] * ctx[5] / ctx[4]) / d["N_b_DFT_os"])
    return np.abs(np.einsum("rtp,pk->rtk", taps["a"], ph))


# ---- the sync -> RX chain: one packet per window through the same channel at 25 dB, with one STF of
# lead-in, as tests/test_gpu_sync.py test_sync_then_demodulate builds its windows
# name: (psdef, ctx, chestim lr, seed)
SYNC_CASES = {
    "tm1_txdiv2": (F.PARITY_CASES["tm1_txdiv2"][0], F.PARITY_CASES["tm1_txdiv2"][1], 1, 4203),
    "r42_qpsk": (G.CASES["r42_qpsk"][0], G.CASES["r42_qpsk"][1], 1, 4202),
}
SYNC_SNR_DB = 25.0


@functools.lru_cache(maxsize=None)
def sync_window(name):
    """dict: win (complex64 [N_RX, S_win], read-only), start (the first tap's hw sample), chunk, pcc, pdc,
    nid, pt, and the oracle configurations (ocf, ops, osc)"""
    psd, ctx, lr, seed = SYNC_CASES[name]
    u_max, b_max, n_rx, os_min, L, M = ctx
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M, lr=lr), O.psdef(*psd)
    sz = O.packet_sizes(ops)
    d = O.dims(ocf, ops)
    S = d["N_packet_os_rs"]
    pre = sz["N_samples_STF"] * os_min * L // M
    S_win = S + pre + 32
    chunk = S_win * 7 // 8
    rng = np.random.default_rng(seed)
    pcc = rng.integers(0, 256, 25, dtype=np.uint8)
    pdc = rng.integers(0, 256, (sz["G"] + 7) // 8, dtype=np.uint8)
    nid, pt = 100, 1
    cfo_dect = rng.uniform(-1.75, 1.75) * 2 * np.pi / d["N_b_DFT_os"]
    # the TX mixer applies the CFO, as phy_fixtures.sync_window does
    x, _ = O.tx(ocf, ops, pcc, pdc, S, network_id=nid, plcf_type=pt, phase_inc=cfo_dect * M / L)
    start = pre + int(rng.integers(0, 32))
    delays, gains = _sync_profile(name)
    win, taps = selective_channel(rng, x, n_rx, S_win, start, 0.0, SYNC_SNR_DB, delays, gains, DOPPLER_CYCLES)
    win.setflags(write=False)
    osc = O.sync_cfg(psd[0], psd[1], os_min=os_min, L=L, M=M, n_ant=n_rx, chunk_len=chunk)
    return dict(win=win, start=start, chunk=chunk, pcc=pcc, pdc=pdc, nid=nid, pt=pt, ocf=ocf, ops=ops, osc=osc,
                psd=psd, ctx=ctx, lr=lr, taps=taps)


def _sync_profile(name):
    psd, ctx, _, _ = SYNC_CASES[name]
    d = O.dims(O.cfg(ctx[0], ctx[1], ctx[3], ctx[4], ctx[5]), O.psdef(*psd))
    D = max(3, int(round(0.58 * d["CP_os"] * ctx[4] / ctx[5] / 2)))
    return (0, int(round(0.17 * D)), int(round(0.56 * D)), D), PROFILE_4
