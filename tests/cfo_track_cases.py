"""Inputs and models shared by tests/test_rx_cfo_track_host.py and tests/test_gpu_rx_cfo_track.py (TEST
INFRASTRUCTURE, no GPU): residual CFO tracking from the DRS symbols (dnrp_ctx_set_rx_cfo_tracking; the intent of
the reference's build option RX_SYNCED_PARAM_CFO_RESIDUAL_BASED_ON_DRS, rx_synced_param.hpp:162-181).

Offset windows. A noise-free oracle-TX packet through sto_track_cases.mixing() is multiplied by
exp(j omega (m - n_stf)) for every DECT-rate sample m at or behind the end of the STF (n_stf = STF_CP +
N_b_DFT_os; at 10/9 the hw-rate sample n is m = n M / L). The STF estimate then sees no offset and the mixer
increment that removes the injected one is inc1 - omega: truth. One DRS period's rotation is
omega step (CP + N_b_DFT_os), `rot` in the case table, at most pi / 2.

The geometries are sto_track_cases.py's (the smallest packets with two DRS symbols per stream set; case c's
three slots hold three). omega = rot / (step (CP + N_b_DFT_os)), rad per DECT-rate sample:
    a         rot 0.45,  step 5,  CP + N_b_DFT_os = 144 (os_min 2):  6.2500e-04
    d         rot 0.9,   step 5,  144 (l mode):                      1.2500e-03
    b         rot 0.45,  step 5,  288:                               3.1250e-04
    c         rot 0.45,  step 10, 288:                               1.5625e-04
    u8b16, C3 rot 0.45,  step 5,  1152:                              7.8125e-05
    C4        rot 0.45,  step 10, 1152:                              3.9063e-05
    u8b16_c4  rot 0.225, step 5,  1152 (the model at C4's omega):    3.9063e-05

The model (L = M = 1 contexts only, where the front end is a slice, a mixer product and an FFT): model_table()
restates the front end of every DRS symbol with the STF values and rx_cfo_track_kernel's recurrence in double
precision numpy.

The pre-rotated input: prerotate() multiplies the samples of symbol l by exp(j (table phase - STF-only
phase)). The mixer is a product in the time domain, so the unchanged oracle receiver on it computes what a
tracking receiver computes on the original window (exact for L = M = 1).

Recorded deviations of the model's increment from the injected truth, as a fraction of omega (equally: of one
DRS period's rotation), measured by tests/test_rx_cfo_track_host.py, which asserts the 20 % cap (DESIGN.md
section 6.9). After the second op of a stream set (the first update):
    a 0.0031  b 0.0081  c 0.0001  d 0.0030  u8b16 0.0018  u8b16_c4 0.0018
the largest over all updates, which MODEL_DEV holds and the GPU bounds are built on:
    a 0.0950  b 0.0917  c 0.0445  d 0.0950  u8b16 0.0853  u8b16_c4 0.0853
The second figure is the loop's own transient, not noise: a DRS symbol is mixed with the entry from before its
update, so the half symbol between its window's centre and the first CP sample of the next symbol
(N_b_DFT_os / 2 of the period's samples: 64 / 720 = 0.089 at step 5, 0.044 at step 10) keeps the old
increment, and the next measurement reads that rotation as a frequency error. With gain 1 the error r_n after update n
follows r_n+1 = q (r_n - r_n-1), q that share: 0, -q omega, -q^2 omega, ... The first figure is the inter-carrier
interference of the offset, proportional to omega as the measured rotation is.
The unchanged oracle on case d's window (l mode, 16-QAM, rot 0.9): BASELINE_D = 0.1054 of the PDC signs of the
packet's last quarter wrong (0.036 at rot 0.45, 0.052 at 0.6: below or at the 5 % the benefit test needs, so d
carries 0.9); the GPU benefit test reproduces that share with tracking off and no error with it on.
"""
import math

import numpy as np

import oracle_py as O
import phy_fixtures as F
import sto_track_cases as ST

# name: rotation per DRS period (rad); psdef, context and channel-estimation mode are sto_track_cases.CASES'
# d: 0.9, where the unchanged oracle's error share in the last quarter is visibly bad (0.036 / 0.052 / 0.105 at
# 0.45 / 0.6 / 0.9; the limit asked for is 0.05); u8b16_c4: C4's omega, whose DRS period is twice the model case's
ROT = {"a": 0.45, "b": 0.45, "c": 0.45, "d": 0.9, "u8b16": 0.45, "u8b16_c4": 0.225, "C3": 0.45, "C4": 0.45}
MODEL_OF = ST.MODEL_OF
MODEL_CASES = ST.MODEL_CASES
# largest |model increment - truth| / omega that tests/test_rx_cfo_track_host.py measured (rounded up); the GPU
# test's bound on the wave front end and the epoch receiver is twice that of the model case at their b and omega
MODEL_DEV = {"a": 0.0950, "b": 0.0917, "c": 0.0445, "d": 0.0950, "u8b16": 0.0853, "u8b16_c4": 0.0853}
MODEL_DEV_FIRST = {"a": 0.0031, "b": 0.0081, "c": 0.0001, "d": 0.0030, "u8b16": 0.0018, "u8b16_c4": 0.0018}
DEV_CAP = ST.DEV_CAP
BASELINE_D = 0.1054  # the host test's measurement, see the docstring
BASELINE_MIN = 0.05


def geometry(name):
    g = dict(ST.geometry(name))
    g["sym"] = g["CP"] + g["Nd"]
    g["rot"] = ROT[name]
    g["omega"] = ROT[name] / (g["step"] * g["sym"])
    return g


def rotate(g, y, omega):
    """the packet y [rows, S] (hw rate, starting at sample 0) turned by exp(j omega (m - n_stf)) from the end
    of the STF on, m = n M / L the DECT-rate position of hw sample n"""
    m = np.arange(y.shape[1], dtype=np.float64) * g["M"] / g["L"]
    ph = np.where(m >= g["n_stf"], omega * (m - g["n_stf"]), 0.0)
    return np.asarray(y, np.complex128) * np.exp(1j * ph)[None, :]


_WIN = {}


def window(name, omega=None, seed=3, off=5, eps=0.0):
    """One noise-free window of a case with the carrier offset omega (and the sampling drift eps of
    sto_track_cases.drift), computed once: dict with win complex64 [N_RX, S], the fine peak `off`, the
    transmitted packed bits, network ID and PLCF type. The sync report carries no CFO."""
    g = geometry(name)
    omega = g["omega"] if omega is None else omega
    key = (name, omega, seed, off, eps)
    if key not in _WIN:
        rng = np.random.default_rng(seed)
        sz, S = g["sz"], g["S"]
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + seed % 6, 1 + seed % 2
        x, _ = O.tx(g["ocf"], g["ops"], pcc, pdc, S, network_id=nid, plcf_type=pt)
        y = rotate(g, ST.mixing(g["n_rx"], x.shape[0]) @ ST.drift(g, x, eps), omega)
        win = np.zeros((g["n_rx"], S), np.complex128)
        win[:, off:] = y[:, :S - off]
        win = win.astype(np.complex64)
        win.setflags(write=False)
        _WIN[key] = dict(win=win, off=off, pcc=pcc, pdc=pdc, nid=nid, pt=pt, omega=omega, eps=eps)
    return _WIN[key]


def model_table(g, win, fp, a0, inc1, inc_sto, gain=1.0):
    """rx_cfo_track_kernel's table [N_DF + 1, 2] (phase a, increment) for an L = M = 1 context in double: the
    front end of every DRS symbol with the STF values (slice, mixer, FFT, bin extraction, amplitude, STF
    derotation), then the recurrence. (a0, inc1): the entry without an update; inc_sto: the STF's STO increment"""
    assert g["L"] == 1 and g["M"] == 1
    Nd, N, n_stf, sym = g["Nd"], g["N"], g["n_stf"], g["sym"]
    kk = np.arange(N + 1)
    bins = np.where(kk >= N // 2, kk - N // 2, g["off_lower"] + kk)
    tab = np.full((g["N_DF"] + 1, 2), np.nan)
    a, run, lf = float(a0), float(inc1), 0
    hist = {}  # first stream -> (symbol, pilots [rx, stream, cell], subcarriers [stream, cell], Psi)
    for l, tf, tl, kmat in g["drs"]:
        tab[lf:l + 1] = (a, run)
        lf = l + 1
        m0 = ST._m0(g, l)
        seg = win[:, fp + m0:fp + m0 + Nd].astype(np.complex128)
        seg = seg * np.exp(1j * (a0 + inc1 * (m0 - n_stf + np.arange(Nd))))[None, :]
        Y = np.fft.fft(seg, axis=1)[:, bins] * (np.sqrt(N) / Nd) * np.exp(1j * inc_sto * (kk - N // 2))[None, :]
        ts = range(tf, min(tl, 7, tf + 3) + 1)
        h = np.stack([Y[:, kmat[t - tf]] * O.drs_values(g["b"], t)[None, :] for t in ts], axis=1)
        psi = (a - a0) + ((l - 1) * sym + g["CP"] + Nd // 2) * (run - inc1)
        if tf in hist:
            lp, hp, kp, psip = hist[tf]
            C = np.sum(h * np.conj(hp))
            for j in range(h.shape[1]):  # per stream: its cells sit two subcarriers above or below the earlier ones
                if kp[j, 0] > kmat[j, 0]:  # the earlier symbol's cell i lies above: the other side is its cell i - 1
                    C += np.sum(h[:, j, 1:] * np.conj(hp[:, j, :-1]))
                elif kp[j, 0] < kmat[j, 0]:
                    C += np.sum(h[:, j, :-1] * np.conj(hp[:, j, 1:]))
            theta = math.remainder(float(np.angle(C)) + psi - psip, 2.0 * math.pi)
            nxt = run - gain * theta / ((l - lp) * sym)
            a += l * sym * (run - nxt)
            run = nxt
        hist[tf] = (l, h, kmat, psi)
    tab[lf:] = (a, run)
    return tab


def updates(g):
    """the DRS symbols after which the increment changes: those with an earlier op of the same stream set"""
    seen, out = set(), []
    for l, tf, _, _ in g["drs"]:
        if tf in seen:
            out.append(l)
        seen.add(tf)
    return out


def model_deviation(g, tab, inc1, omega=None):
    """largest |increment behind an updating DRS symbol - truth| over those that have a symbol behind them, as
    a fraction of omega (= of one DRS period's rotation)"""
    omega = g["omega"] if omega is None else omega
    dev = 0.0
    for l in updates(g):
        if l + 1 <= g["N_DF"] and np.isfinite(tab[l + 1, 1]):
            dev = max(dev, abs(tab[l + 1, 1] - (inc1 - omega)))
    return dev / abs(omega)


def first_deviation(g, tab, inc1, omega=None):
    """|increment behind the second op of a stream set - truth| / omega, the largest over the stream sets"""
    omega = g["omega"] if omega is None else omega
    seen, dev = {}, 0.0
    for l, tf, _, _ in g["drs"]:
        seen[tf] = seen.get(tf, 0) + 1
        if seen[tf] == 2:
            dev = max(dev, abs(tab[l + 1, 1] - (inc1 - omega)))
    return dev / abs(omega)


def table_diff(g, tab, model):
    """largest |device - model| over the table as a fraction of one DRS period's rotation: the increments over
    one period's samples, and the phases"""
    n = g["N_DF"] + 1
    period = g["step"] * g["sym"]
    d_inc = float(np.max(np.abs(tab[:n, 1] - model[:, 1]))) * period
    d_a = float(np.max(np.abs(tab[:n, 0] - model[:, 0])))
    return max(d_inc, d_a) / g["rot"]


def prerotate(g, win, fp, tab):
    """the window with the samples of every symbol (CP included) turned by that symbol's table phase - STF-only
    phase; tab[1] is the entry without an update"""
    assert g["L"] == 1 and g["M"] == 1
    out = win.astype(np.complex128)
    a0, inc1 = tab[1]
    for l in range(1, g["N_DF"] + 1):
        if not np.all(np.isfinite(tab[l])) or (tab[l, 0] == a0 and tab[l, 1] == inc1):
            continue
        mm = np.arange((l - 1) * g["sym"], l * g["sym"])  # m - n_stf
        s = fp + g["n_stf"] + mm
        out[:, s] *= np.exp(1j * ((tab[l, 0] - a0) + mm * (tab[l, 1] - inc1)))[None, :]
    return out.astype(np.complex64)


last_quarter_errors = ST.last_quarter_errors
inc_of_sto = ST.inc_of_sto
