"""Inputs and the model shared by tests/test_rx_mimo_report_host.py and tests/test_gpu_rx_mimo_report.py (TEST
INFRASTRUCTURE, no GPU): the MIMO report options (dnrp_ctx_set_rx_mimo_report, dnrp_rx_mimo_detail;
kernels/rx_mimo.hip rx_mimo_detail_kernel).

The model restates, in double precision numpy, the single-stream codebook search of estimator_mimo.cpp:162-271
under its three metrics and both search starts (search()), and the rank / precoder report for spatial
multiplexing (rates(), report()): per wideband cell He = H_c W scaling, G = He^H He + nv I,
r_c = sum_i -log2(nv [G^-1]_ii), the candidate's rate the mean over the 4 cells. W and the scaling factors come
from the library's own literal tables (dnrp.query_table).

Windows are built like sto_track_cases.window: an oracle-TX packet through codebook 0, times a seeded
N_RX x N_TX mixing, at offset 5, no CFO, plus white noise 20 dB below each RX antenna's own signal power, so the
noise variance is well above the floor 2^-14 P and G is well conditioned.
"""
import numpy as np

import oracle_py as O
import phy_fixtures as F

NONE = 0xFFFFFFFF
MAX_CB = 28
A_NONZERO = {2: 2, 4: 12}  # first single-stream entry without a zero element
SCORE_CAP, RATE_CAP = 1.0e-4, 1.0e-3  # the loosest bounds the GPU test may use (units of the packet's largest)
SNR_DB = 20.0
N_PACKETS = 8

# name: psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_RX, os_min, L, M); lr 1 throughout
GEOMETRIES = {
    "t2r2": ((2, 2, 1, 2, 1, 3), (2, 2, 2, 2, 1, 1)),
    "t4r4": ((1, 2, 1, 3, 5, 3), (1, 2, 4, 2, 1, 1)),
    "t2r4": ((1, 2, 1, 3, 1, 3), (1, 2, 4, 2, 1, 1)),
    "t1r2": ((2, 2, 1, 2, 0, 3), (2, 2, 2, 2, 1, 1)),
    "t2r8": ((1, 1, 1, 2, 1, 3), (1, 1, 8, 2, 1, 1)),  # no reciprocal codebook at 8 antennas
    # the paths test's geometry (sto_track_cases C4) and the spatial-multiplexing packet of TX_ONLY_CASES tm2_sm2
    "C4": ((8, 16, 1, 1, 5, 1), (8, 16, 4, 1, 10, 9)),
    "tm2_sm2": F.TX_ONLY_CASES["tm2_sm2"][:2],
}
BATCH_GEOMETRIES = ("t2r2", "t4r4", "t2r4", "t1r2", "t2r8")


def geometry(name):
    psd, ctx = GEOMETRIES[name]
    u_max, b_max, n_rx, os_min, L, M = ctx
    ocf, ops = O.cfg(u_max, b_max, os_min, L, M, lr=1), O.psdef(*psd)
    sz, d = O.packet_sizes(ops), O.dims(ocf, ops)
    return dict(name=name, psd=psd, ctx=ctx, lr=1, ocf=ocf, ops=ops, sz=sz, n_rx=n_rx, n_ts=sz["N_eff_TX"], n_tx=sz["N_TX"],
                S=d["N_packet_os_rs"])


# ---------------------------------------------------------------- tables
_W = {}


def codebook(R, N):
    """(W complex [ncb, N, R] as [antenna][layer], scaling [ncb]) of W_t's codebook (N_SS R, N_TX N); None if W_t
    has none for the rank report (N outside {1, 2, 4} or R > N)"""
    import dnrp
    if N not in (1, 2, 4) or R > N or R not in (1, 2, 4):
        return None
    if (R, N) not in _W:
        ncb = int(dnrp.query_table("W_codebooks", R, N)[0])
        W = np.stack([dnrp.query_table("W", R, N, cb).astype(np.float64).view(np.complex128).reshape(N, R) for cb in range(ncb)])
        sc = np.array([float(dnrp.query_table("W_scaling", R, N, cb)[0]) for cb in range(ncb)])
        _W[(R, N)] = (W, sc)
    return _W[(R, N)]


# ---------------------------------------------------------------- mixings
def gauss(seed, n_rx, n_tx):
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal((n_rx, n_tx)) + 1j * rng.standard_normal((n_rx, n_tx))) / np.sqrt(2.0)


def rank_one(g, n_tx, cb):
    """g w_cb^H, w_cb the single-stream entry cb of the codebook (1, n_tx) times its scaling: the entry that
    matches it is cb"""
    W, sc = codebook(1, n_tx)
    return np.outer(np.asarray(g, np.complex128), np.conj(W[cb, :, 0] * sc[cb]))


def unitary(n):
    k = np.arange(n)
    return np.exp(-2j * np.pi * np.outer(k, k) / n) / np.sqrt(n)


# ---------------------------------------------------------------- the model
def _better(metric):
    return (lambda a, b: a < b) if metric == 2 else (lambda a, b: a > b)


def search(H, side, metric, all_w):
    """estimator_mimo.cpp:162-271 on the stage H [N_RX, N_TS, 4]: side "tx" searches the codebook (1, N_TS) over
    the RX antennas, "rx" the codebook (1, N_RX) over the transmit streams (the transposed stage). Returns
    (index, scores [28] with NaN where not scored, margin): margin is |best - second| of the scored entries
    (inf with fewer than two, or where the decision is the same in any arithmetic)."""
    H = np.asarray(H, np.complex128)
    Hs = H if side == "tx" else np.transpose(H, (1, 0, 2))  # [receive side, transmit side, cell]
    n_rxv, n_txv = Hs.shape[0], Hs.shape[1]
    scores = np.full(MAX_CB, np.nan)
    if n_txv == 1:
        return 0, scores, np.inf
    if n_txv not in A_NONZERO:
        return NONE, scores, np.inf
    W, sc = codebook(1, n_txv)
    A = 0 if all_w else A_NONZERO[n_txv]
    better = _better(metric)
    best, idx = (1.0e6 if metric == 2 else -1.0e6), NONE
    for wm in range(A, len(sc)):
        p = np.abs(np.einsum("rtc,t->r", Hs, W[wm, :, 0]))
        inner = p.min() if metric == 0 else p.sum() if metric == 1 else p.max() - p.min()
        scores[wm] = inner * sc[wm]
        if better(scores[wm], best):
            best, idx = scores[wm], wm
    s = np.sort(scores[np.isfinite(scores)])
    margin = np.inf if len(s) < 2 else (s[1] - s[0] if metric == 2 else s[-1] - s[-2])
    if metric == 2 and n_rxv == 1:
        margin = np.inf  # max - min of one value: every spread is exactly 0 in any arithmetic, the search start wins
    return idx, scores, float(margin)


def first_best(scores, metric):
    """the first best of a score vector as the search picks it (NaN entries are not candidates)"""
    better = _better(metric)
    best, idx = (1.0e6 if metric == 2 else -1.0e6), NONE
    for wm, s in enumerate(scores):
        if np.isfinite(s) and better(s, best):
            best, idx = s, wm
    return idx


def nv_used(nv, H, n_rx, n_ts):
    """max(nv, 2^-14 P, FLT_MIN), P the mean |H|^2 of the N_RX N_TS 4 stage entries"""
    P = float(np.mean(np.abs(np.asarray(H, np.complex128)[:n_rx, :n_ts, :]) ** 2))
    return max(float(nv), 2.0 ** -14 * P, float(np.finfo(np.float32).tiny))


def rates(H, nv):
    """rate_cb [3, 28] (NaN where there is no candidate) on the stage H [N_RX, N_TS, 4] with noise variance nv"""
    H = np.asarray(H, np.complex128)
    n_rx, n_ts = H.shape[0], H.shape[1]
    out = np.full((3, MAX_CB), np.nan)
    for s, R in enumerate((1, 2, 4)):
        cbk = codebook(R, n_ts) if R <= min(n_ts, n_rx) else None
        if cbk is None:
            continue
        W, sc = cbk
        for cb in range(len(sc)):
            r = 0.0
            for c in range(4):
                He = H[:, :, c] @ W[cb] * sc[cb]
                Gi = np.linalg.inv(He.conj().T @ He + nv * np.eye(R))
                r += float(np.sum(-np.log2(nv * np.real(np.diag(Gi)))))
            out[s, cb] = r / 4.0
    return out


def report(rate_cb):
    """(pmi [3], rate [3], RI, PMI, sinr_eff_dB, margins [4]) that rate_cb implies: the first maximum per rank
    slot, the rank with the largest rate (ties to the lower); margins: top-two of each slot's candidates, then
    of the ranks' rates (inf with fewer than two)"""
    pmi, rate, RI, PMI, best = [NONE] * 3, [np.nan] * 3, 0, NONE, None
    margins = []
    for s in range(3):
        v = np.asarray(rate_cb[s], np.float64)
        fin = np.isfinite(v)
        if not fin.any():
            margins.append(np.inf)
            continue
        pmi[s] = int(np.argmax(np.where(fin, v, -np.inf)))
        rate[s] = float(v[pmi[s]])
        t = np.sort(v[fin])
        margins.append(np.inf if len(t) < 2 else float(t[-1] - t[-2]))
        if best is None or rate[s] > best:
            RI, PMI, best = 1 << s, pmi[s], rate[s]
    t = np.sort([r for r in rate if np.isfinite(r)])
    margins.append(np.inf if len(t) < 2 else float(t[-1] - t[-2]))
    sinr = 10.0 * np.log10(2.0 ** (best / RI) - 1.0) if RI else np.nan
    return pmi, rate, RI, PMI, sinr, margins


# ---------------------------------------------------------------- windows
_WIN = {}


def window(name, mix, seed=0, off=5, snr_db=SNR_DB):
    """One window of geometry `name`, computed once per (name, mix key): mix is ("gauss", seed), ("rank_one", cb,
    seed) or ("unitary",). dict with win complex64 [N_RX, S], the fine peak `off`, network ID, PLCF type and the
    mixing."""
    key = (name, mix, seed, off, snr_db)
    if key not in _WIN:
        g = geometry(name)
        rng = np.random.default_rng(7000 + seed)
        sz, S = g["sz"], g["S"]
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + seed % 6, 1 + seed % 2
        x, _ = O.tx(g["ocf"], g["ops"], pcc, pdc, S, network_id=nid, plcf_type=pt)
        M = mixing(g, mix)
        y = M @ x.astype(np.complex128)
        win = np.zeros((g["n_rx"], S), np.complex128)
        win[:, off:] = y[:, :S - off]
        sigma = np.sqrt(np.mean(np.abs(y) ** 2, axis=1) / 10.0 ** (snr_db / 10.0) / 2.0)
        win += sigma[:, None] * (rng.standard_normal(win.shape) + 1j * rng.standard_normal(win.shape))
        win = win.astype(np.complex64)
        win.setflags(write=False)
        _WIN[key] = dict(win=win, off=off, nid=nid, pt=pt, mix=M)
    return _WIN[key]


def mixing(g, mix):
    n_rx, n_tx = g["n_rx"], g["n_tx"]
    if mix[0] == "gauss":
        return gauss(mix[1], n_rx, n_tx)
    if mix[0] == "unitary":
        assert n_rx == n_tx
        return unitary(n_rx)
    if mix[0] == "rank_one":
        gv = gauss(mix[2], n_rx, 1)[:, 0]
        # Antenna 0 is 14 dB above the others. The stage is the zero-forced pilot, so every entry carries an
        # error of its antenna's noise variance, and a rank-2 candidate whose first column matches w sees a
        # phantom second layer through those errors: it loses 1 bit to the power split and gains about
        # log2(1 + (N_RX - 1) e / (2 nv)), e the error variance of the antennas beside the strongest. With equal
        # gains e = nv and 4 antennas that is 1.3 bits, a coin toss against rank 1. The noise here is 20 dB below
        # each antenna's own power and nv is the mean over the antennas, so e / nv = 0.04 / 0.28 and the phantom
        # layer is worth 0.3 bits at most: rank 1 wins by more than half a bit.
        gv = gv / np.abs(gv) * np.where(np.arange(n_rx) == 0, 1.0, 0.2)
        return rank_one(gv, n_tx, mix[1])
    raise KeyError(mix)


def batch(name):
    """the geometry's batch: N_PACKETS windows with gauss seeds 0..N_PACKETS-1"""
    return [window(name, ("gauss", s), seed=s) for s in range(N_PACKETS)]


def stage_of(M):
    """the mixing itself as the stage, constant over the 4 cells"""
    return np.repeat(np.asarray(M, np.complex128)[:, :, None], 4, axis=2)
