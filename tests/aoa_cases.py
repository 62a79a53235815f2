"""Inputs and models shared by tests/test_rx_aoa_host.py and tests/test_gpu_rx_aoa.py (TEST INFRASTRUCTURE, no
GPU): the angle-of-arrival report from the DRS pilots (dnrp_ctx_set_rx_aoa, dnrp_rx_aoa, dnrp_aoa_estimate;
DESIGN.md §6.11; the reference's estimator_aoa_t has empty bodies).

Windows. An oracle-TX packet x [N_TX, S] reaches antenna r as a_r(az) (g^T x), a(az) the array's steering vector and
g a fixed vector of equal-magnitude entries (one plane wave: a rank-one channel, whatever the number of transmit
streams), placed at sample `off` of the window; optional seeded noise. The sync report carries `off` and zero CFO.

estimate(): the definition restated in double numpy (steering table, Bartlett scan, first maximum, three-point
parabola, first-lag sum) on a covariance rounded to complex64, as the device stores it.

model_cov(): for L = M = 1 contexts, the front end of every DRS symbol the way sto_track_cases.model_table builds
it (slice, mixer with the device's cfo_fine, FFT, bin extraction, amplitude, DRS values), then R = sum h h^H in
double. The STO derotation has unit modulus per subcarrier and cancels in every product; it is left out.

NOISY_ERR_DEG: |az of the model's R - truth| of every noisy case at 10 dB, measured by tests/test_rx_aoa_host.py on
the model alone (it gates at twice the figure, and so does nothing looser than the inputs' own decidability).
BIAS_DEG: the restatement's worst interpolation error on exact a a^H (same test).
"""
import numpy as np

import oracle_py as O
import phy_fixtures as F

TWO_PI = 2.0 * np.pi
SPAN_TOL = 1e-5
NONE = 0xFFFFFFFF


def ula(n, d=0.5):
    """n antennas d wavelengths apart along y: a_r = exp(j 2 pi r d sin az), unambiguous over +-90 deg"""
    return np.array([(0.0, r * d) for r in range(n)], np.float32)


def uca(n, radius=0.6):
    ph = TWO_PI * np.arange(n) / n
    return np.stack([radius * np.cos(ph), radius * np.sin(ph)], axis=1).astype(np.float32)


HALF_PI = float(np.float32(np.pi / 2))
PI_F = float(np.float32(np.pi))
SCAN_ULA = (-HALF_PI, HALF_PI, 181)
SCAN_UCA = (-PI_F, PI_F, 360)  # cyclic: the span is 2 pi within the float rounding of the end points

# name: psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_RX, os_min, L, M), antenna positions, scan, the
# packets' true azimuths in degrees, PDC requests (PCC-batch slots in request order), environment, receiver mode
CASES = {
    # NRX 2, one stream, 14 cells per op
    "ula2": dict(psd=(1, 1, 1, 2, 0, 3), ctx=(1, 1, 2, 2, 1, 1), pos=ula(2), scan=SCAN_ULA, az=(20.0,), req=(0,)),
    # NRX 4, four streams, two ops per DRS period; three packets requested as (2, 0): rows follow the requests
    "ula4_td": dict(psd=(1, 2, 1, 3, 5, 3), ctx=(1, 2, 4, 2, 1, 1), pos=ula(4), scan=SCAN_ULA, az=(-50.0, 10.0, 65.0),
                    req=(2, 0)),
    # NRX 8, 36 pairs, the parabola's neighbours wrap at grid index 0
    "uca8": dict(psd=(1, 1, 1, 2, 0, 3), ctx=(1, 1, 8, 2, 1, 1), pos=uca(8), scan=SCAN_UCA, az=(-179.7,), req=(0,)),
    # the default epoch receiver at 10/9, and the plain Y path on the same packet
    "c4": dict(psd=(8, 16, 1, 1, 5, 1), ctx=(8, 16, 4, 1, 10, 9), pos=ula(4), scan=SCAN_ULA, az=(33.0,), req=(0,)),
    "c4_y": dict(psd=(8, 16, 1, 1, 5, 1), ctx=(8, 16, 4, 1, 10, 9), pos=ula(4), scan=SCAN_ULA, az=(33.0,), req=(0,),
                 env=dict(DNRP_RX_EPOCH="0", DNRP_RX_FUSED="1")),
    # both residual trackers on
    "ula4_td_track": dict(psd=(1, 2, 1, 3, 5, 3), ctx=(1, 2, 4, 2, 1, 1), pos=ula(4), scan=SCAN_ULA,
                          az=(-50.0, 10.0, 65.0), req=(2, 0), track=True),
    # the MMSE receiver of spatial multiplexing (rx_grid_cases sm42_16qam's psdef and context)
    "sm42": dict(psd=(1, 1, 0, 1, 2, 3), ctx=(1, 1, 4, 1, 10, 9), pos=ula(4), scan=SCAN_ULA, az=(-20.0,), req=(0,),
                 sm=True),
}
MODEL_CASES = ("ula2", "ula4_td", "uca8")  # L = M = 1
NOISY_SNR_DB = 10.0
# measured by tests/test_rx_aoa_host.py (printed there): per case the largest |az(model R) - truth| in degrees
NOISY_ERR_DEG = {"ula2": 0.168, "ula4_td": 0.119, "uca8": 0.040}
# the restatement's worst |az - truth| on exact a a^H in degrees: 181 points over +-90 deg, |az| <= 75 deg, N_RX 2, 4,
# 8 line arrays; the 360-point cyclic scan on the 8-antenna circle
BIAS_DEG = {"ula": 0.0325, "uca": 0.0002}
BIAS_CAP_DEG = {"ula": 0.05, "uca": 0.001}


def bias_kind(name):
    return "uca" if name.startswith("uca") else "ula"


def geometry(name):
    c = CASES[name]
    u_max, b_max, n_rx, os_min, L, M = c["ctx"]
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M), O.psdef(*c["psd"])
    sz, d = O.packet_sizes(ops), O.dims(ocf, ops)
    g = dict(c, name=name, ocf=ocf, ops=ops, sz=sz, n_rx=n_rx, L=L, M=M, Nd=d["N_b_DFT_os"], CP=d["CP_os"],
             STF_CP=d["STF_CP_os"], off_lower=d["off_lower"], N=sz["N_b_OCC"], N_DF=sz["N_DF_symb"],
             S=d["N_packet_os_rs"], b=c["psd"][1], env=c.get("env", {}), track=c.get("track", False), sm=c.get("sm", False))
    g["n_stf"] = g["STF_CP"] + g["Nd"]
    g["drs"] = O.drs_cells(c["psd"][1], sz["N_TS"], sz["N_DF_symb"])
    g["n_cells"] = sum((tl - tf + 1) * k.shape[1] for _, tf, tl, k in g["drs"])
    return g


# ---------------------------------------------------------------- the definition in numpy
def steering(pos, az):
    """a_r(az) for pos [n, 2] (wavelengths) and az [...] (rad): [..., n] complex128"""
    pos = np.asarray(pos, np.float32).astype(np.float64)
    az = np.asarray(az, np.float64)
    return np.exp(1j * TWO_PI * (np.cos(az)[..., None] * pos[:, 0] + np.sin(az)[..., None] * pos[:, 1]))


def grid(az_min, az_max, n_grid):
    """(az [n_grid], step, cyclic) from the float32 end points"""
    lo, hi = float(np.float32(az_min)), float(np.float32(az_max))
    span = hi - lo
    cyclic = abs(span - TWO_PI) <= SPAN_TOL
    step = TWO_PI / n_grid if cyclic else span / (n_grid - 1)
    return lo + np.arange(n_grid) * step, step, cyclic


def estimate(pos, az_min, az_max, n_grid, R, n_rx=None, conj=False):
    """The report's fields behind R from R [n, n] (rounded to complex64 first): dict with grid_idx, az_rad, peak
    (double, and az32 / peak32 as the report rounds them), lag, spectrum (double). conj: a wrong model that
    conjugates the steering vector (test only)."""
    n = len(pos) if n_rx is None else n_rx
    R = np.asarray(R)[:n, :n].astype(np.complex64).astype(np.complex128)
    az, step, cyclic = grid(az_min, az_max, n_grid)
    A = steering(np.asarray(pos)[:n], az)
    if conj:
        A = A.conj()
    tr = float(np.sum(np.real(np.diag(R))))
    lag = complex(np.sum(np.diag(R, -1)))
    if not tr > 0.0:
        return dict(grid_idx=NONE, az_rad=0.0, peak=0.0, az32=np.float32(0), peak32=np.float32(0), lag=lag,
                    spectrum=np.zeros(n_grid))
    P = np.real(np.einsum("gr,rc,gc->g", A.conj(), R, A)) / (n * tr)
    i = int(np.argmax(P))  # the first maximum
    a, pk = az[i], P[i]
    if cyclic or 0 < i < n_grid - 1:
        ym, yp = P[(i - 1) % n_grid], P[(i + 1) % n_grid]
        den = ym - 2.0 * pk + yp
        if den < 0.0:
            dl = min(0.5, max(-0.5, 0.5 * (ym - yp) / den))
            a = a + dl * step
            pk = pk - 0.25 * (ym - yp) * dl
            if cyclic and a < az[0]:
                a += TWO_PI
    return dict(grid_idx=i, az_rad=float(a), peak=float(pk), az32=np.float32(a), peak32=np.float32(pk), lag=lag, spectrum=P)


def ang_err_deg(az_rad, truth_deg):
    """|az - truth| in degrees, modulo a full turn"""
    d = np.rad2deg(float(az_rad)) - truth_deg
    return abs((d + 180.0) % 360.0 - 180.0)


# ---------------------------------------------------------------- windows
def tx_weights(n_tx):
    t = np.arange(n_tx)
    return np.exp(TWO_PI * 1j * (0.23 * t + 0.07 * t * t)) / np.sqrt(n_tx)


_WIN = {}


def windows(name, snr_db=None, seed=7, off=5):
    """The case's windows, computed once: list of dicts with win complex64 [N_RX, S] (read-only), off, the
    transmitted packed bits, network ID, PLCF type and the true azimuth in degrees. snr_db None: noise-free."""
    key = (name, snr_db, seed, off)
    if key not in _WIN:
        g = geometry(name)
        out = []
        for i, az_deg in enumerate(g["az"]):
            rng = np.random.default_rng(seed + 17 * i)
            sz, S = g["sz"], g["S"]
            pcc = O.pack_bits(F.random_bits(rng, 196))
            pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
            nid, pt = 100 + (seed + i) % 6, 1 + (seed + i) % 2
            x, _ = O.tx(g["ocf"], g["ops"], pcc, pdc, S, network_id=nid, plcf_type=pt)
            x = np.asarray(x).astype(np.complex128)
            s = tx_weights(x.shape[0]) @ x
            y = steering(g["pos"], np.deg2rad(az_deg))[:, None] * s[None, :]
            win = np.zeros((g["n_rx"], S), np.complex128)
            win[:, off:] = y[:, :S - off]
            if snr_db is not None:
                sigma = np.sqrt(np.mean(np.abs(s) ** 2) / 10.0 ** (snr_db / 10.0) / 2.0)
                win += sigma * (rng.standard_normal(win.shape) + 1j * rng.standard_normal(win.shape))
            win = win.astype(np.complex64)
            win.setflags(write=False)
            out.append(dict(win=win, off=off, pcc=pcc, pdc=pdc, nid=nid, pt=pt, az_deg=az_deg))
        _WIN[key] = out
    return _WIN[key]


# ---------------------------------------------------------------- pilot model (L = M = 1)
def model_cov(g, win, fp, cfo_fine=0.0, swap=None):
    """R [N_RX, N_RX] complex128 of one window as rx_aoa_kernel defines it, from a double front end. swap: a
    wrong model that exchanges two antennas' rows (test only)."""
    assert g["L"] == 1 and g["M"] == 1
    Nd, N, n_stf = g["Nd"], g["N"], g["n_stf"]
    kk = np.arange(N + 1)
    bins = np.where(kk >= N // 2, kk - N // 2, g["off_lower"] + kk)
    n = win.shape[0]
    R = np.zeros((n, n), np.complex128)
    for l, tf, tl, kmat in g["drs"]:
        m0 = n_stf + (l - 1) * (g["CP"] + Nd) + g["CP"]
        seg = win[:, fp + m0:fp + m0 + Nd].astype(np.complex128)
        seg = seg * np.exp(1j * cfo_fine * (m0 - n_stf + np.arange(Nd)))[None, :]
        Y = np.fft.fft(seg, axis=1)[:, bins] * (np.sqrt(N) / Nd)
        for t in range(tf, tl + 1):
            h = Y[:, kmat[t - tf]] * O.drs_values(g["b"], t)[None, :]
            R += h @ h.conj().T
    if swap is not None:
        p = list(range(n))
        p[swap[0]], p[swap[1]] = p[swap[1]], p[swap[0]]
        R = R[np.ix_(p, p)]
    return R
