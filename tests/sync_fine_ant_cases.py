"""Inputs shared by tests/test_sync_fine_ant_host.py and tests/test_gpu_sync_fine_ant.py (TEST INFRASTRUCTURE):
oracle-TX packets in the window of a receiver of class (u, b_max, os_min, L, M) with n_ant antennas, and the
all-antenna fine search of crosscorrelator_t::run_fine_search (crosscorrelator.cpp:137-147, 165-248) restated
in numpy (double): per antenna the direct dot products of the CFO-rotated hw-rate samples against the STF
templates of dnrp_query_table("sync_template"), then the metric sums, the first largest sum and the
metric-weighted mean index.

Every window: MCS 1, one random N_RX x N_TX mixing per packet, a CFO within +-1.75 subcarriers, the packet
start at least two STFs into the window, 30 dB unless a variant says otherwise. The windows are a pure
function of their case (seeded), so both files see the same samples.
"""
import zlib

import numpy as np

import oracle_py as O
import phy_fixtures as F
import sync_beta_cases as K

RTOL_METRIC = 1e-3  # tests/test_gpu_sync.py:54: fine_peak_metric against the oracle, rtol=1e-3
N_WINDOWS = 2

# (u, b_max, os_min, L, M, n_ant, tm): the smallest that reach every form of the fine search
CASES = [(1, 1, 1, 1, 1, 2, 1),     # 256-point, in-place radix 4
         (1, 2, 1, 1, 1, 2, 1),     # 512-point, Stockham
         (1, 4, 1, 10, 9, 4, 5),    # resampled stream, four antennas, three templates
         (1, 16, 1, 1, 1, 2, 1),    # 4096-point radix-8 form of C3 / C4
         (2, 8, 1, 1, 1, 8, 10),    # eight antennas, four templates
         (2, 12, 2, 10, 9, 2, 1)]   # 8192-point Stockham (131 KB of LDS per workgroup), os_min 2
FOUR = CASES[2]
# variants of FOUR: per-antenna delay in hw samples, per-antenna SNR in dB against the antenna's own packet
# power (None: the common 30 dB against the mean power), the antenna that carries noise only
VARIANTS = {
    "a": dict(delay=(0, 3, 1, 2), snr=None, silent=None),   # the weighted index differs from the strongest antenna's
    "b": dict(delay=(0, 0, 0, 0), snr=None, silent=3),      # noise only, -40 dB against the others' packet power
    "c": dict(delay=(3, 0, 0, 0), snr=(30.0, 10.0, 10.0, 10.0), silent=None),  # the strongest antenna is the late one
}
SILENT_DB = -40.0
# added to a case's seed: the first value with which every window of the case meets the margin conditions of
# tests/test_sync_fine_ant_host.py (the peak of a template that was not transmitted is a maximum of noise-like
# lags, and two of those can lie within the margin of each other)
SALT = {((2, 8, 1, 1, 1, 8, 10), None): 174, ((1, 4, 1, 10, 9, 4, 5), "a"): 3, ((1, 4, 1, 10, 9, 4, 5), "b"): 90,
        ((1, 4, 1, 10, 9, 4, 5), "c"): 1}


def case_id(c):
    return "u%d_b%d_os%d_%d_%d_ant%d_tm%d" % c


def c8(c, b=None):
    """the case as a tuple of tests/sync_beta_cases.py: the packet's b is the class' unless given"""
    return tuple(c) + (c[1] if b is None else b,)


def psdef(c):
    """MCS 1, the shortest packet the transmission mode has: one slot, two at u = 1 from four transmit streams on"""
    u, b_max, _, _, _, _, tm = c
    return (u, b_max, 1, 2 if u == 1 and tm >= 5 else 1, tm, 1)


def geometry(c):
    """Sizes of a case: the packet's slot length and STF length in hw samples (tests/sync_beta_cases.py::geometry)"""
    u, b_max, os_min, L, M, _, _ = c
    S = O.dims(O.cfg(u, b_max, os_min=os_min, L=L, M=M), O.psdef(*psdef(c)))["N_packet_os_rs"]
    N = 64 * b_max * os_min
    stf_hw = (N + N // 4 * (3 if u == 1 else 5)) * L // M
    return dict(S=S, stf_hw=stf_hw, S_win=2 * stf_hw + 32 + S + stf_hw)


def chunk_len(c):
    return geometry(c)["S_win"] * 7 // 8


def packet(rng, c, cfo_dect_rad, i=0):
    """One oracle-TX packet of the case, mixed onto the case's antennas: (y [n_ant, S], meta)."""
    u, b_max, os_min, L, M, n_ant, _ = c
    cf, ps = O.cfg(u, b_max, os_min=os_min, L=L, M=M), O.psdef(*psdef(c))
    pcc = rng.integers(0, 256, 25, dtype=np.uint8)
    pdc = rng.integers(0, 256, (O.packet_sizes(ps)["G"] + 7) // 8, dtype=np.uint8)
    nid, pt = 100 + i % 6, 1 + i % 2
    x, _ = O.tx(cf, ps, pcc, pdc, geometry(c)["S"], network_id=nid, plcf_type=pt, phase_inc=cfo_dect_rad * M / L)
    return F.mixing_matrix(rng, n_ant, x.shape[0]) @ x, (pcc, pdc, nid, pt)


def sync_geometry(c):
    u, b_max, os_min, L, M, n_ant, _ = c
    return O.sync_geometry(O.sync_cfg(u, b_max, os_min=os_min, L=L, M=M, n_ant=n_ant))


def oracle_sync_cfg(c, n_lim=None):
    u, b_max, os_min, L, M, n_ant, _ = c
    return O.sync_cfg(u, b_max, os_min=os_min, L=L, M=M, n_ant=n_ant, n_lim=n_lim, chunk_len=chunk_len(c))


_CACHE = {}


def windows(c, variant=None):
    """The N_WINDOWS windows of a case: list of (window complex64 [n_ant, S_win], start, meta, delays)."""
    key = (c, variant)
    if key in _CACHE:
        return _CACHE[key]
    v = VARIANTS[variant] if variant else dict(delay=(0,) * c[5], snr=None, silent=None)
    rng = np.random.default_rng(zlib.crc32((case_id(c) + (variant or "")).encode()) + SALT.get(key, 0))
    g = geometry(c)
    out = []
    for i in range(N_WINDOWS):
        start, cfo = 2 * g["stf_hw"] + int(rng.integers(0, 32)), K.draw_cfo(rng, c8(c))
        y, meta = packet(rng, c, cfo, i)
        half = y[:, : g["S"] // 2]
        p_ant = np.mean(np.abs(half) ** 2, axis=1)
        p_mean = float(np.mean(np.abs(half) ** 2))
        win = np.zeros((c[5], g["S_win"]), np.complex128)
        sigma = np.empty(c[5])
        for a in range(c[5]):
            if a != v["silent"]:
                win[a, start + v["delay"][a]: start + v["delay"][a] + g["S"]] = y[a]
            if a == v["silent"]:
                sigma[a] = np.sqrt(p_mean * 10 ** (SILENT_DB / 10) / 2)
            elif v["snr"] is None:
                sigma[a] = np.sqrt(p_mean / 10 ** (K.SNR_DB / 10) / 2)
            else:
                sigma[a] = np.sqrt(p_ant[a] / 10 ** (v["snr"][a] / 10) / 2)
        noise = rng.standard_normal(win.shape) + 1j * rng.standard_normal(win.shape)
        out.append(((win + sigma[:, None] * noise).astype(np.complex64), start, meta, v["delay"]))
    _CACHE[key] = out
    return out


# both settings on: a b = 1 packet in the stream of a b_max = 4 receiver with two antennas, the windows of
# tests/sync_beta_cases.py (PARITY)
BETA_CASE = (1, 4, 1, 1, 1, 2, 1, 1)


def two_packet_window(c, seed=81):
    """one window holding two packets of the case, for the ring of rx_sync_stream: (window, [start, start])"""
    rng = np.random.default_rng(seed)
    g = geometry(c)
    starts = [2 * g["stf_hw"] + 11, 2 * g["stf_hw"] + 11 + g["S"] + 3 * g["stf_hw"] + 5]
    win = np.zeros((c[5], starts[1] + g["S"] + g["stf_hw"]), np.complex128)
    p = []
    for i, st in enumerate(starts):
        y, _ = packet(rng, c, K.draw_cfo(rng, c8(c)), i)
        win[:, st:st + g["S"]] += y
        p.append(np.mean(np.abs(y[:, : g["S"] // 2]) ** 2))
    return K.add_noise(rng, win, np.mean(p)), starts


_TMPL = {}


def templates(c, b=None):
    """the fine search's time-domain templates of a b packet in the case's stream, complex128 [n_templates, tmpl_len]"""
    import dnrp
    u, b_max, os_min, L, M, _, _ = c
    key = (u, b_max, os_min, L, M, c[5], b or b_max)
    if key not in _TMPL:
        nt = sync_geometry(c)["n_templates"]
        _TMPL[key] = np.stack([dnrp.query_table("sync_template", u, b_max, os_min, L, M, b or b_max, 1 << k)
                               .view(np.complex64).astype(np.complex128) for k in range(nt)])
    return _TMPL[key]


def antenna_xcorr(win, c, coarse_time, cfo_frac, a, b=None):
    """|cross-correlation| of antenna a over the xc_len lags against every template, float64 [n_templates, xc_len]
    (crosscorrelator.cpp:173-188): the hw-rate samples from coarse_time - xc_l (zero outside the window) rotated
    by exp(j cfo_hw i), cfo_hw = cfo_frac M / L, conjugate dot products of tmpl_len samples per lag."""
    g = sync_geometry(c)
    T = templates(c, b)
    assert T.shape[1] == g["tmpl_len"]
    n = g["xc_len"] - 1 + g["tmpl_len"]
    base = int(coarse_time) - g["xc_l"]
    q = base + np.arange(n)
    ok = (q >= 0) & (q < win.shape[1])
    s = np.zeros(n, np.complex128)
    s[ok] = win[a, q[ok]]
    s *= np.exp(1j * (float(cfo_frac) * c[4] / c[3]) * np.arange(n))
    return np.stack([np.abs(np.correlate(s, t, "valid")) for t in T])


def antenna_peaks(win, c, coarse_time, cfo_frac, coarse_array, n_lim=None, b=None):
    """peak_vec of crosscorrelator.cpp:190-201 for every processed antenna: (metric float64 [8, 4], index int64
    [8, 4] relative to the search start, xcorr {antenna: [n_templates, xc_len]}); 0 where not processed."""
    metric, index, xc = np.zeros((8, 4)), np.zeros((8, 4), np.int64), {}
    for a in range(n_lim or c[5]):
        if not coarse_array[a] > 0:
            continue
        xc[a] = antenna_xcorr(win, c, coarse_time, cfo_frac, a, b)
        for k, r in enumerate(xc[a]):
            index[a, k] = int(np.argmax(r))  # first maximum (volk_32fc_index_max_32u)
            metric[a, k] = r[index[a, k]]
    return metric, index, xc


def combine(metric, index, coarse_array, n_templates, n_lim=8):
    """crosscorrelator.cpp:218-248 on a per-antenna table, in double: (metric_sum [n_templates], the weighted
    mean index x [n_templates] before rounding, k_likely)"""
    ants = [a for a in range(n_lim) if coarse_array[a] > 0]
    ms = np.array([sum(float(metric[a, k]) for a in ants) for k in range(n_templates)])
    x = np.array([sum(float(metric[a, k]) * float(index[a, k]) for a in ants) / ms[k] for k in range(n_templates)])
    k_likely, best = 0, 0.0
    for k in range(n_templates):
        if best < ms[k]:  # strictly larger: ties go to the first template
            best, k_likely = ms[k], k
    return ms, x, k_likely


def strongest(coarse_array, n_lim):
    """the antenna the search takes with the setting off: first maximum of coarse_peak_array (ant.cpp:104-108)"""
    return int(np.argmax(np.asarray(coarse_array[:n_lim])))
