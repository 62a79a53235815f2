"""Inputs shared by tests/test_sync_edges_host.py and tests/test_gpu_sync_edges.py (TEST INFRASTRUCTURE): sync
windows at the edges the other sync suites stay away from. Every number is written out; the host file proves
from the oracle alone (oracle_py.sync_trace) that each case reaches the branch its `kind` names and keeps its
margin, the GPU file holds the kernels to the oracle on the identical windows.

Classes (Case.cls) and kinds (Case.kind):
  position    one packet, its start swept over the head of the window (kinds head_none / head_found: the
              oracle's ignore_before = stf_len + pattern and its "STF before the chunk" drop) and over the tail
              of the search (tail_found / tail_none: search_len = A + 4 STF)
  truncation  one packet at a fixed start in S_full samples, the same samples cut to S_win: cut_steps (the last
              step sums read past the window), cut_fine (the fine-search stage does), cut_coarse (the coarse
              search range does), cut_stf (the cut lies inside the STF); each with an odd S_win twin, and
              noise-free twins whose tail has exactly zero power
  gates       antennas scaled below rms_min (x 1e-3), above SYNC_RMS_MAX (x 50) or to exactly zero; one live
              antenna of four; N_ant_limited = 2 of 4 with a stronger packet on the unsearched antennas
  backtoback  two C2 packets, the second 0 / 50 / 150 / 400 samples after the first slot ends, and one pair
              overlapping in time
The layout class (LAYOUTS) reads the position windows of two configurations through other strides and
alignments, the stream class (STREAM_*) sweeps one packet across a chunk boundary of rx_sync_stream.

A window is a pure function of its case: default_rng(seed) draws the CFO (+-1.75 subcarriers), then
phy_fixtures.sync_window the payload, the N_RX x N_TX mixing and the noise (30 dB unless the case says otherwise).
"""
import collections
import functools

import numpy as np

import oracle_py as O
import phy_fixtures as F

Case = collections.namedtuple("Case", "id cls kind name S_full S_win chunk starts seed gains snr_db n_lim hidden max_reports")


def _case(id, cls, kind, name, S_full, S_win, chunk, starts, seed, gains=None, snr_db=30.0, n_lim=None, hidden=None,
          max_reports=2):
    return Case(id, cls, kind, name, S_full, S_win, chunk, tuple(starts), seed, gains, snr_db, n_lim, hidden, max_reports)


# ---- geometry of the configurations used (hw samples), for the reader; the host file checks them
#   name               step  stf_hw  ignore_hw  search_hw  S_full  chunk  step-sum form
#   C2                    4     124        142        897    1500    400  sync_steps_stream_kernel<.., 0>
#   C3                   64    2560       2844      14330   20480   4096  pipe / stream-16 / wave (FORMS)
#   lm1_1_u8b16          64    2304       2560      13312   20480   4096  sync_steps_kernel <1, 1, 0> (tiles)
#   lm40_27_u8b12_tm5    48    2560       2844      14320   20480   4096  sync_steps_kernel <0, 0, 0>, 4 antennas
#   os2_u2b2_tm1         16     640        711       3760    6000   1200  sync_steps_kernel <9, 10, 4>, 2 antennas
#   tm1_txdiv2           32    1280       1422       7680   12800   2560  2 antennas
#   mrc4_16qam           16     640        711       3760    6000   1200  4 antennas
SIZES = {"C2": (1500, 400), "C3": (20480, 4096), "lm1_1_u8b16": (20480, 4096), "lm40_27_u8b12_tm5": (20480, 4096),
         "os2_u2b2_tm1": (6000, 1200), "tm1_txdiv2": (12800, 2560), "mrc4_16qam": (6000, 1200)}

# environments a configuration's windows run under on the GPU (the step-sum and detection forms)
FORMS = {
    "C2": [{}],
    "C3": [{}, {"DNRP_SYNC_PIPE": "0"}, {"DNRP_SYNC_STREAM": "0"}, {"DNRP_SYNC_ROUNDS": "0"}, {"DNRP_SYNC_ROUNDS": "2"}],
    "lm1_1_u8b16": [{}],
    "lm40_27_u8b12_tm5": [{}],
    "os2_u2b2_tm1": [{}],
    "tm1_txdiv2": [{}],
    "mrc4_16qam": [{}],
}


def _position(name, kind, starts, seed0):
    """starts: hw samples, or (start, seed) where the case keeps a seed of its own"""
    S, chunk = SIZES[name]
    pairs = [st if isinstance(st, tuple) else (st, seed0 + i) for i, st in enumerate(starts)]
    return [_case("pos_%s_%d" % (name, st), "position", kind, name, S, S, chunk, [st], seed) for st, seed in pairs]


# the expected count (0 or 1) is the oracle's; the kind says which side of which edge the start lies on
POSITION = (
    _position("C2", "head_none", [1, 3, (2, 702), (4, 704)], 500)
    + _position("C2", "head_found", [20, 40, 60, 124, 130, 143, 160], 510)
    + _position("C2", "tail_found", [660, 700, 730, 760, (840, 721), (855, 723)], 520)
    + _position("C2", "tail_none", [(880, 534), 870, 900, 940], 530)
    + _position("C3", "head_none", [40], 540)
    + _position("C3", "head_found", [1200, 2900], 541)
    + _position("C3", "tail_found", [10000, 11500], 543)
    + _position("C3", "tail_none", [14400], 545)
    + _position("os2_u2b2_tm1", "head_none", [10], 550)
    + _position("os2_u2b2_tm1", "head_found", [300, 730], 551)
    + _position("os2_u2b2_tm1", "tail_found", [2600, 3000], 553)
    + _position("os2_u2b2_tm1", "tail_none", [3800], 555)
)


def _cuts(name, start, cuts, seed, noise_free=()):
    """cuts: {kind: S_win}; every cut also with the odd S_win next to it, the kinds of noise_free once more with
    snr_db = None (zero samples outside the packet, so the cut tail has exactly zero power)"""
    S, chunk = SIZES[name]
    out = []
    for kind, s_win in cuts.items():
        for sw in (s_win, s_win - 1 if s_win % 2 == 0 else s_win + 1):
            out.append(_case("cut_%s_%s_%d" % (name, kind[4:], sw), "truncation", kind, name, S, sw, chunk, [start], seed))
        if kind in noise_free:
            out.append(_case("cut_%s_%s_%d_clean" % (name, kind[4:], s_win), "truncation", kind, name, S, s_win, chunk,
                             [start], seed, snr_db=None))
    return out


# cut_steps of C2 keeps the packet whole (60 + 800 <= 880 < 897): the chain test demodulates it
TRUNCATION = (
    _cuts("C2", 60, {"cut_steps": 880, "cut_fine": 190, "cut_coarse": 174, "cut_stf": 148}, 560,
          noise_free=("cut_coarse",))
    + _cuts("C3", 4096, {"cut_steps": 14000, "cut_fine": 6920, "cut_coarse": 6700, "cut_stf": 6000}, 561,
            noise_free=("cut_coarse", "cut_stf"))
    + _cuts("lm1_1_u8b16", 4096, {"cut_steps": 13000, "cut_fine": 6630, "cut_coarse": 6400, "cut_stf": 5700}, 562)
    + _cuts("lm40_27_u8b12_tm5", 4096, {"cut_steps": 14000, "cut_fine": 6920, "cut_coarse": 6700, "cut_stf": 6000}, 563)
    + _cuts("os2_u2b2_tm1", 1200, {"cut_steps": 3700, "cut_fine": 1906, "cut_coarse": 1850, "cut_stf": 1650}, 564)
)


def _gates(name, start, seed):
    S, chunk = SIZES[name]
    n = F.case(name)[1][2]
    out = []
    for which, a in (("first", 0), ("last", n - 1)):
        for kind, g in (("gate_rms_min", 1e-3), ("gate_rms_max", 50.0), ("gate_zero", 0.0)):
            gains = tuple(g if i == a else 1.0 for i in range(n))
            out.append(_case("%s_%s_%s" % (kind, name, which), "gates", kind, name, S, S, chunk, [start], seed, gains=gains))
    return out


GATES = (
    _gates("tm1_txdiv2", 2500, 570)
    + _gates("mrc4_16qam", 1200, 571)
    # every gate at once: antenna 3 alone is live
    + [_case("gate_one_live_of_4", "gates", "gate_one_live", "mrc4_16qam", 6000, 6000, 1200, [1200], 572,
             gains=(0.0, 1e-3, 50.0, 1.0))]
    # antennas 2 and 3 hold a packet of 1.5 x the amplitude (its RMS stays below SYNC_RMS_MAX) at 400, which a
    # search of antennas 0 and 1 must not see
    + [_case("gate_n_lim_2_of_4", "gates", "gate_n_lim", "mrc4_16qam", 6000, 6000, 1200, [2200], 573, n_lim=2,
             hidden=(400, 1.5))]
    # a window long enough for the whole packet (slot 6400): the chain test demodulates it
    + [_case("gate_zero_mrc4_16qam_whole", "gates", "gate_zero", "mrc4_16qam", 8000, 8000, 1200, [1200], 574,
             gains=(0.0, 1.0, 1.0, 1.0))]
)
CHAIN = ("cut_C2_steps_880", "gate_zero_mrc4_16qam_whole")
GATES_ZERO = [c for c in GATES if c.kind in ("gate_zero", "gate_one_live")]  # also run with the all-antenna fine search
GATES_ICFO = "gate_zero_tm1_txdiv2_first"                                     # also run with the integer CFO search

# C2 slot: 800 hw samples. First packet at 300, so its slot ends at 1100.
BACKTOBACK = [_case("b2b_gap_%d" % gap, "backtoback", "b2b_gap", "C2", 3000, 3000, 3000, [300, 1100 + gap], 580 + i,
                    max_reports=4) for i, gap in enumerate((0, 50, 150, 400))]
BACKTOBACK += [_case("b2b_overlap", "backtoback", "b2b_overlap", "C2", 3000, 3000, 3000, [300, 900], 585, max_reports=4)]

CASES = POSITION + TRUNCATION + GATES + BACKTOBACK
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# ---- layouts: the position windows of these configurations (LAYOUT_NAMES) read four ways; the reports equal
# those of the same windows in the plain layout [n][n_ant][S], every row 16-byte aligned
LAYOUT_NAMES = ("C2", "os2_u2b2_tm1")
LAYOUTS = ("offset1",   # a flat tensor sliced [1:]: the base 8 bytes into a 16-byte unit, strides as plain
           "odd",       # S_win - 1 samples per row (odd), contiguous: every other row 8 bytes off
           "overlap",   # one linear stream per antenna, win_stride = chunk_len < S_win, ant_stride = its length
           "pad3")      # ant_stride = S_win + 3


def layout_windows(name):
    return [window(c)[0] for c in POSITION if c.name == name]


# ---- stream sweep: C2 through rx_sync_stream, chunk 400, one packet per run in a noise ring (25 dB), its start
# swept from boundary - 2 STF to boundary + 2 STF (STF = 124 hw samples) around the chunk boundary 1600
STREAM_CHUNK, STREAM_N_CHUNKS, STREAM_BOUNDARY, STREAM_MAX_REPORTS = 400, 8, 1600, 3
STREAM_S_WIN = 1836  # dnrp_sync_stream_window of C2 at chunk 400 (the GPU file checks it)
STREAM_STARTS = [1352, 1394, 1435, 1476, 1518, 1559, 1590, 1600, 1610, 1641, 1683, 1724, 1766, 1807, 1848]
STREAM_UNIQUE_LIMIT = 16  # one STF pattern at b = 1, os_min = 1
O_UNDEFINED_EARLY = np.iinfo(np.int64).min // 8


def stream_ring(start, seed=None):
    """(ring complex64 [1, R], g0): the global time g0 of stream sample 0 lies so that the ring wraps inside the
    searched range; the packet starts at stream sample `start`"""
    rng = np.random.default_rng(600 + start if seed is None else seed)
    T = STREAM_N_CHUNKS * STREAM_CHUNK + STREAM_S_WIN
    cfo = rng.uniform(-1.2, 1.2) * 2 * np.pi / 64
    pkt, _ = F.sync_window(rng, O, "C2", 900, [0], cfo, snr_db=None)
    stream = np.zeros((1, T), np.complex64)
    stream[:, start:start + 900] += pkt
    sigma = np.sqrt(np.mean(np.abs(pkt[pkt != 0]) ** 2) / 10 ** 2.5 / 2)
    stream = (stream + sigma * (rng.standard_normal(stream.shape) + 1j * rng.standard_normal(stream.shape))).astype(np.complex64)
    g0 = 5 * T + T // 3
    ring = np.zeros((1, T), np.complex64)
    ring[:, (g0 + np.arange(T)) % T] = stream
    return ring, g0


def stream_oracle(ring, g0, use_float=False):
    """numpy gather + oracle search per chunk + the baton's uniqueness test in chunk order (the checker of
    tests/test_gpu_stream.py::_oracle_stream, restated here so that the host file needs no torch):
    ([(global fine peak, chunk, report)], double detections)"""
    osc = O.sync_cfg(1, 1, n_ant=1, chunk_len=STREAM_CHUNK)
    R = ring.shape[1]
    last, out, dup = O_UNDEFINED_EARLY, [], 0
    for k in range(STREAM_N_CHUNKS):
        tk = g0 + k * STREAM_CHUNK
        win = ring[:, (np.arange(STREAM_S_WIN) + tk) % R]
        for r in O.sync(osc, win, max_reports=STREAM_MAX_REPORTS, use_float=use_float):
            t = tk + r["fine_64"]
            if t - last > STREAM_UNIQUE_LIMIT:
                last = t
                out.append((t, k, r))
            else:
                dup += 1
    return out, dup


# ---- windows and the oracle on them
def sync_cfg(c, chunk=None):
    psd, (_, _, n_ant, os_min, L, M) = F.case(c.name)
    return O.sync_cfg(psd[0], psd[1], os_min=os_min, L=L, M=M, n_ant=n_ant, n_lim=c.n_lim, chunk_len=chunk or c.chunk)


def geometry(c):
    return O.sync_geometry(sync_cfg(c))


def n_eff_tx(c):
    return O.packet_sizes(O.psdef(*F.case(c.name)[0]))["N_eff_TX"]


def _build(c, seed, cut=True):
    rng = np.random.default_rng(seed)
    psd, cfgt = F.case(c.name)
    cfo = rng.uniform(-1.75, 1.75) * 2 * np.pi / (64 * psd[1] * cfgt[3])
    win, meta = F.sync_window(rng, O, c.name, c.S_full, list(c.starts), cfo, snr_db=c.snr_db)
    if c.hidden is not None:  # the unsearched antennas hold another, stronger packet instead
        other, _ = F.sync_window(rng, O, c.name, c.S_full, [c.hidden[0]], -cfo, snr_db=c.snr_db)
        win[c.n_lim:] = np.float32(c.hidden[1]) * other[c.n_lim:]
    if c.gains is not None:
        win = win * np.asarray(c.gains, np.float32)[:, None]
    return np.ascontiguousarray(win[:, :c.S_win if cut else c.S_full]), meta


@functools.lru_cache(maxsize=None)
def _window(cid):
    return _build(BY_ID[cid], BY_ID[cid].seed)


def window(c):
    """(window complex64 [n_ant, S_win], [(pcc_d, pdc_d, network_id, plcf_type)]); shared, leave unchanged"""
    return _window(c.id)


def searched(c, win):
    """the rows the search is given: all of them, or the first N_ant_limited"""
    return win if c.n_lim is None else win[:c.n_lim]


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    c = BY_ID[cid]
    return O.sync_trace(sync_cfg(c), searched(c, window(c)[0]), max_reports=c.max_reports)


def oracle(c):
    """(reports, trace) of the oracle's double path on the case's window, computed once"""
    return _oracle(c.id)


def second_seed(c):
    """the same case with every draw from another seed (payload, mixing, noise)"""
    return _build(c, c.seed + 1000)[0]


def uncut(c):
    """the window before the cut: what a kernel that reads past S_win would see"""
    return _build(c, c.seed, cut=False)[0]
