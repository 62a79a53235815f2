"""Inputs and models shared by tests/test_rx_sto_track_host.py and tests/test_gpu_rx_sto_track.py (TEST
INFRASTRUCTURE, no GPU): residual STO tracking from the DRS symbols (dnrp_ctx_set_rx_sto_tracking; the
reference's build option RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS, estimator_sto.cpp:64-97, 148-171).

Drifted windows. An oracle-TX packet x is resampled by 1 + eps with a Kaiser-windowed sinc interpolator
(taps_of() taps, at least 64, double): y[n] = x(n - eps (n - c)) behind the STF, c the centre of the STF's transform window,
and y[n] = x[n] inside the STF, so the STF estimate sees no drift and the delay of symbol l (at the centre of
its transform window) is eps l (CP + N_b_DFT_os) samples. eps > 0 delays: a transform window then slides
into its own cyclic prefix (an advance would take in the next symbol's, inter-symbol interference that grows
with the accumulated drift). A delay of d samples turns the pilots by
exp(-j 2 pi d k / N_b_DFT_os) over the signed subcarrier k; the receiver derotates by exp(j inc (k_index -
N_b_OCC / 2)) (estimator_sto.cpp:163-171 convert_to_phasors), so the increment that removes it is
inc = 2 pi d / N_b_DFT_os: truth_inc(). One DRS period's drift is that value for `step` symbols.

The model (L = M = 1 contexts only, where the front end is a slice and an FFT): model_table() restates the
front end of every DRS symbol and rx_sto_track_kernel's recurrence in double precision numpy.

The pre-rotated input: prerotate() turns the content of every symbol's transform window by that symbol's
table - STF increment, in frequency. The unchanged oracle receiver (STF-only STO) on it computes what a
tracking receiver computes on the original window.

Recorded deviations of the model from the injected truth, as a fraction of one DRS period's drift (measured
by tests/test_rx_sto_track_host.py, which asserts the 20 % cap):
    a 0.0226  b 0.0240  c 0.0089  d 0.0226  u8b16 0.0524  u8b16_c4 0.0446
a / d: the DC-straddling pilot pair, 5 subcarriers apart and divided by 4, about 1 / (4 (n_drs - 1)) = 1.9 % of a
residual at b = 1. u8b16: the delayed symbol boundaries ring into the transform window (band-limited delay).
The oracle without tracking on case b's window (the longest): 0.0003 of the PDC signs of the packet's last
quarter wrong (16-QAM, noise-free; its time interpolation between DRS symbols absorbs a linear drift).
"""
import numpy as np

import oracle_py as O
import phy_fixtures as F

KAISER_BETA = 12.0


def taps_of(os_min, L, M):
    """interpolator taps: the transition band of the Kaiser-windowed sinc, 0.12 / 0.06 / 0.03 of the sample
    rate for 64 / 128 / 256 taps, must end above the signal's band edge 0.4375 L / (M os_min)"""
    return 64 if os_min >= 2 else 128 if L > M else 256


# name: psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_RX, os_min, L, M), chestim lr, eps
# a..d: L = M = 1 at os_min = 2 (the signal well inside the band); u8b16: the lm1_1_u8b16 geometry, the
# model's reference for the C3 geometry, u8b16_c4 for C4's (same b and eps); C3 / C4: the wave front end and
# the epoch receiver at 10/9, one packet. These carry QPSK: the update after a DRS symbol leaves the data
# symbols behind it up to 0.8 of one period's drift away from the pilots they are equalised with (the DRS
# symbol itself is derotated with the value from before), 0.5 rad at the band edge for these eps (C4's DRS
# period is twice C3's), which QPSK signs survive and 256-QAM signs do not. A smaller eps puts the deviation
# from the truth above what the model allows: the band-limited delay rings across the symbol boundaries, and
# at 10/9 the images the 14 dB resamplers leave act as noise on the pilots, neither of which shrinks with eps
# (C3 measured 0.20 / 0.10 / 0.06 of a period at eps 1e-5 / 2e-5 / 4e-5; C4 averages 16 angles: 0.007)
CASES = {
    "a": ((1, 1, 1, 2, 0, 3), (1, 1, 1, 2, 1, 1), 1, 1.0e-3),
    "b": ((2, 2, 1, 2, 1, 3), (2, 2, 2, 2, 1, 1), 1, 5.0e-4),
    "c": ((1, 2, 1, 3, 5, 3), (1, 2, 4, 2, 1, 1), 1, 5.0e-4),
    "d": ((1, 1, 1, 2, 0, 3), (1, 1, 1, 2, 1, 1), 0, 1.0e-3),
    "u8b16": ((8, 16, 1, 1, 0, 1), (8, 16, 1, 1, 1, 1), 1, 4.0e-5),
    "u8b16_c4": ((8, 16, 1, 1, 0, 1), (8, 16, 1, 1, 1, 1), 1, 2.0e-5),
    "C3": ((8, 16, 1, 1, 0, 1), (8, 16, 1, 1, 10, 9), 1, 4.0e-5),
    "C4": ((8, 16, 1, 1, 5, 1), (8, 16, 4, 1, 10, 9), 1, 2.0e-5),
}
MODEL_OF = {"C3": "u8b16", "C4": "u8b16_c4"}  # the model case at the same b and eps
MODEL_CASES = ("a", "b", "c", "d", "u8b16", "u8b16_c4")
# largest |model - truth| / one period's drift that tests/test_rx_sto_track_host.py measured (the docstring's
# figures, rounded up); the GPU test's bound on the wave front end and the epoch receiver is twice that of
# the model case at their b and eps (MODEL_OF)
MODEL_DEV = {"a": 0.0226, "b": 0.0240, "c": 0.0089, "d": 0.0226, "u8b16": 0.0524, "u8b16_c4": 0.0446}
DEV_CAP = 0.20


def geometry(name):
    psd, ctx, lr, eps = CASES[name]
    u_max, b_max, n_rx, os_min, L, M = ctx
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M, lr=lr), O.psdef(*psd)
    sz, d = O.packet_sizes(ops), O.dims(ocf, ops)
    g = dict(name=name, psd=psd, ctx=ctx, lr=lr, eps=eps, ocf=ocf, ops=ops, sz=sz, n_rx=n_rx, L=L, M=M,
             Nd=d["N_b_DFT_os"], CP=d["CP_os"], STF_CP=d["STF_CP_os"], off_lower=d["off_lower"], N=sz["N_b_OCC"],
             N_DF=sz["N_DF_symb"], S=d["N_packet_os_rs"], b=psd[1])
    g["n_stf"] = g["STF_CP"] + g["Nd"]
    g["drs"] = O.drs_cells(psd[1], sz["N_TS"], sz["N_DF_symb"])
    g["step"] = 5 if sz["N_eff_TX"] <= 2 else 10
    return g


def truth_inc(g, l, eps=None):
    """the increment (on top of the STF's) that removes the injected delay of symbol l"""
    eps = g["eps"] if eps is None else eps
    return 2.0 * np.pi * eps * l * (g["CP"] + g["Nd"]) / g["Nd"]


def period_drift(g, eps=None):
    return abs(truth_inc(g, g["step"], eps))


def resample(x, t, taps):
    """x complex [rows, S] at the positions t (in samples of x, zero outside it): Kaiser-windowed sinc"""
    x = np.asarray(x, np.complex128)
    S, half = x.shape[1], taps // 2
    j = np.arange(-half + 1, half + 1)
    out = np.zeros((x.shape[0], len(t)), np.complex128)
    for c0 in range(0, len(t), 8192):
        tc = t[c0:c0 + 8192]
        base = np.floor(tc).astype(np.int64)
        arg = (tc - base)[:, None] - j[None, :]
        w = np.sinc(arg) * np.i0(KAISER_BETA * np.sqrt(np.clip(1.0 - (arg / half) ** 2, 0.0, None))) / np.i0(KAISER_BETA)
        idx = base[:, None] + j[None, :]
        w = np.where((idx >= 0) & (idx < S), w, 0.0)
        out[:, c0:c0 + len(tc)] = np.einsum("rnj,nj->rn", x[:, np.clip(idx, 0, S - 1)], w)
    return out


def drift(g, x, eps):
    """the packet x [N_TX, S] (hw rate, starting at sample 0) with the STF as it is and everything behind it
    resampled by 1 + eps about the STF's centre"""
    r = g["L"] / g["M"]  # hw samples per DECT-rate sample
    n = np.arange(x.shape[1], dtype=np.float64)
    c = (g["STF_CP"] + g["Nd"] / 2) * r
    t = np.where(n < g["n_stf"] * r, n, n - eps * (n - c))
    return resample(x, t, taps_of(g["ctx"][3], g["L"], g["M"])) if eps else np.asarray(x, np.complex128)


def mixing(n_rx, n_tx):
    """a fixed N_RX x N_TX mixing with entries of equal magnitude: the estimator averages the angles of every
    (antenna, stream) unweighted, so a weak entry of a random matrix would let the interference of the data
    cells, which is proportional to eps as the drift is, dominate the mean"""
    a, t = np.arange(n_rx)[:, None], np.arange(n_tx)[None, :]
    return np.exp(2j * np.pi * (a * t / n_rx + 0.1 * a + 0.23 * t)) / np.sqrt(n_tx)


_WIN = {}


def window(name, eps=None, seed=3, off=5):
    """One noise-free drifted window of a case, computed once: dict with win complex64 [N_RX, S], the fine peak
    `off`, the transmitted packed bits, network ID and PLCF type. No CFO: the sync report carries 0."""
    g = geometry(name)
    eps = g["eps"] if eps is None else eps
    key = (name, eps, seed, off)
    if key not in _WIN:
        rng = np.random.default_rng(seed)
        sz, S = g["sz"], g["S"]
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + seed % 6, 1 + seed % 2
        x, _ = O.tx(g["ocf"], g["ops"], pcc, pdc, S, network_id=nid, plcf_type=pt)
        y = mixing(g["n_rx"], x.shape[0]) @ drift(g, x, eps)
        win = np.zeros((g["n_rx"], S), np.complex128)
        win[:, off:] = y[:, :S - off]
        win = win.astype(np.complex64)
        win.setflags(write=False)
        _WIN[key] = dict(win=win, off=off, pcc=pcc, pdc=pdc, nid=nid, pt=pt, eps=eps)
    return _WIN[key]


def _m0(g, l):
    return g["n_stf"] + (l - 1) * (g["CP"] + g["Nd"]) + g["CP"]


def model_table(g, win, fp, inc_stf, cfo_fine=0.0, gain=1.0):
    """rx_sto_track_kernel's table [N_DF + 1] for an L = M = 1 context in double: the front end of every DRS
    symbol (slice, mixer, FFT, bin extraction, amplitude, STF derotation), then the recurrence"""
    assert g["L"] == 1 and g["M"] == 1
    Nd, N, n_stf = g["Nd"], g["N"], g["n_stf"]
    kk = np.arange(N + 1)
    bins = np.where(kk >= N // 2, kk - N // 2, g["off_lower"] + kk)
    tab = np.full(g["N_DF"] + 1, np.nan)
    run, lf = float(inc_stf), 0
    for l, tf, tl, kmat in g["drs"]:
        tab[lf:l + 1] = run
        lf = l + 1
        m0 = _m0(g, l)
        seg = win[:, fp + m0:fp + m0 + Nd].astype(np.complex128)
        seg = seg * np.exp(1j * cfo_fine * (m0 - n_stf + np.arange(Nd)))[None, :]
        Y = np.fft.fft(seg, axis=1)[:, bins] * (np.sqrt(N) / Nd) * np.exp(1j * inc_stf * (kk - N // 2))[None, :]
        delta = run - inc_stf
        ang = []
        for a in range(win.shape[0]):
            for t in range(tf, min(tl, 7) + 1):
                k = kmat[t - tf]
                h = Y[a, k] * O.drs_values(g["b"], t) * np.exp(1j * delta * (k - N // 2))
                ang.append(np.angle(np.sum(h[:-1] * np.conj(h[1:]))) / 4.0)
        if ang:
            run += gain * float(np.mean(ang))
    tab[lf:] = run
    return tab


def model_deviation(g, tab, eps=None):
    """largest |table after a DRS symbol - truth at that symbol| over the DRS symbols that have a symbol behind
    them, as a fraction of one DRS period's drift; tab[0] is the STF increment"""
    dev = 0.0
    for l, _, _, _ in g["drs"]:
        if l + 1 <= g["N_DF"] and np.isfinite(tab[l + 1]):
            dev = max(dev, abs(tab[l + 1] - tab[0] - truth_inc(g, l, eps)))
    return dev / period_drift(g, eps)


def prerotate(g, win, fp, tab):
    """the window with every symbol's transform window turned by that symbol's table - STF increment"""
    assert g["L"] == 1 and g["M"] == 1
    Nd = g["Nd"]
    out = win.astype(np.complex128)
    ks = np.fft.fftfreq(Nd, 1.0 / Nd)  # signed bin index
    for l in range(1, g["N_DF"] + 1):
        if not np.isfinite(tab[l]) or tab[l] == tab[0]:
            continue
        m0 = fp + _m0(g, l)
        out[:, m0:m0 + Nd] = np.fft.ifft(np.fft.fft(out[:, m0:m0 + Nd], axis=1) * np.exp(1j * (tab[l] - tab[0]) * ks)[None, :],
                                         axis=1)
    return out.astype(np.complex64)


def inc_of_sto(g, sto_fractional):
    """rx_pkt_state::sto_inc from the reported sto_fractional (|inc| < pi)"""
    return float(sto_fractional) * 2.0 * np.pi / g["Nd"]


def last_quarter_errors(g, w, llr):
    """share of PDC sign errors against the transmitted bits in the packet's last quarter"""
    G = g["sz"]["G"]
    bits = np.unpackbits(w["pdc"])[:G]
    q = slice(3 * G // 4, G)
    return float(np.mean(bits[q] != (np.asarray(llr)[:G][q] > 0)))
