"""Inputs shared by tests/test_sync_icfo_host.py and tests/test_gpu_sync_icfo.py (TEST INFRASTRUCTURE): oracle-TX
packets with a carrier offset of (4 k + f) subcarriers of the class rate, k the integer part the search of
dnrp_ctx_set_sync_icfo_search has to find and f within +-1.75 the part cfo_fractional_rad carries, and the
estimator restated in numpy (double).

Windows are built as tests/sync_beta_cases.py builds them (30 dB, MCS 1, one random N_RX x N_TX mixing per packet,
the packet at least two STFs into the window), N_WINDOWS per (case, k), seeded by the case and k.
"""
import zlib

import numpy as np

import oracle_py as O
import sync_beta_cases as K

N_WINDOWS = 2
MAX_RANGE = 4
COLS = 2 * MAX_RANGE + 1


class Case:
    """c = (u, b_max, os_min, L, M, n_ant, tm, b) as in sync_beta_cases; rng the search range; ks the injected k;
    beta / fine_all: the other two context settings of the synchronisation."""

    def __init__(self, c, rng, ks, beta=False, fine_all=False):
        self.c, self.rng, self.ks, self.beta, self.fine_all = c, rng, tuple(ks), beta, fine_all

    @property
    def N(self):
        return 64 * self.c[1] * self.c[2]

    @property
    def id(self):
        return K.case_id(self.c) + "_r%d" % self.rng + ("_beta" if self.beta else "") + ("_all" if self.fine_all else "")


BASE = Case((1, 1, 2, 1, 1, 1, 0, 1), 2, range(-2, 3))                     # N = 128
TWO_TX = Case((1, 1, 2, 1, 1, 2, 1, 1), 2, range(-2, 3))                   # N_eff_TX = 2: the STF sequence rotated
# N_eff_TX = 4, 9 patterns, the full range, b < b_max: the cells are those of the decided b
WIDE = Case((2, 8, 1, 1, 1, 4, 5, 1), 4, (-4, -1, 0, 3), beta=True)
WITH_BETA = Case((1, 4, 1, 1, 1, 2, 1, 2), 2, (-2, -1, 1, 2), beta=True)   # both decisions together
CLIPPED = Case((1, 2, 1, 1, 1, 1, 0, 2), 4, (-1, 0, 1))                    # only |k| <= 1 searched
NONE = Case((1, 1, 1, 1, 1, 1, 0, 1), 4, (0,))                             # no candidate but 0 is searched
RESAMPLED = Case((1, 1, 2, 10, 9, 2, 1, 1), 1, (-1, 0, 1))                 # sync_icfo_kernel<9, 10, ...>
COMBINE = Case((1, 1, 2, 1, 1, 2, 1, 1), 2, (-1, 1), fine_all=True)        # the combine kernel writes cfo_int
CASES = [BASE, TWO_TX, WIDE, WITH_BETA, CLIPPED, NONE, RESAMPLED, COMBINE]
HOST_CASES = [q for q in CASES if q.c[3] == q.c[4] == 1 and not q.fine_all]  # COMBINE's windows are TWO_TX's


def searched(N, b, k):
    """a candidate whose outermost cell 4 (7 b + |k|) would reach N / 2 is not searched"""
    return 4 * (7 * b + abs(k)) < N // 2


def rad_of(k, N):
    """cfo_integer_rad of a decided k: a correction, the sign of cfo_fractional_rad; +0 for k = 0"""
    return np.float32(0.0) if k == 0 else np.float32(-k * 8 * np.pi / N)


_CACHE = {}


def windows(q, k):
    """The N_WINDOWS windows of (case, k): list of (window complex64 [n_ant, S_win], start, meta, f_rad)."""
    key = (q.c, k)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(("icfo_%s_k%d" % (K.case_id(q.c), k)).encode()))
        g, out = K.geometry(q.c), []
        for i in range(N_WINDOWS):
            start, f = 2 * g["stf_hw"] + int(rng.integers(0, 32)), K.draw_cfo(rng, q.c)
            y, meta = K.packet(rng, q.c, f + 4 * k * 2 * np.pi / q.N, i)
            win = np.zeros((q.c[5], g["S_win"]), np.complex128)
            win[:, start:start + g["S"]] = y
            out.append((K.add_noise(rng, win, np.mean(np.abs(y[:, : g["S"] // 2]) ** 2)), start, meta, f))
        _CACHE[key] = out
    return _CACHE[key]


def all_windows(q):
    """[(k, window, start, meta)] of a case, k-major"""
    return [(k, w[0], w[1], w[2]) for k in q.ks for w in windows(q, k)]


def derotate(win, k, N):
    """the window with 4 k subcarriers of the class rate taken out (L = M = 1: class rate = window rate)"""
    n = np.arange(win.shape[1])
    return (win.astype(np.complex128) * np.exp(-1j * 8 * np.pi * k / N * n)).astype(np.complex64)


def scores(x, u, N, b, at, cfo_frac, rng):
    """The estimator in double: x [n_ant, S] class-rate samples, `at` the coarse peak, cfo_frac the report's
    fractional CFO (a correction). Returns [n_ant, COLS], column k + MAX_RANGE, -1 where k is outside the range or
    not searched: the power of the N-point transform of the STF's last N samples, cover sequence and fractional CFO
    taken out, on the bins 4 (i + k), 0 < |i| <= 7 b."""
    n_pattern = 7 if u == 1 else 9
    cp = N // 4 * (n_pattern - 4)
    seg = np.zeros((x.shape[0], N), np.complex128)
    have = x[:, at + cp: at + cp + N]
    seg[:, : have.shape[1]] = have
    i = np.arange(N)
    cover = O.cover_sequence().astype(np.float64)[n_pattern - 4 + i // (N // 4)]
    P = np.abs(np.fft.fft(seg * cover * np.exp(1j * float(cfo_frac) * i), axis=1)) ** 2
    cell = np.array([c for c in range(-7 * b, 7 * b + 1) if c != 0])
    out = -np.ones((x.shape[0], COLS))
    for k in range(-rng, rng + 1):
        if searched(N, b, k):
            out[:, k + MAX_RANGE] = P[:, (4 * (cell + k)) % N].sum(1)
    return out


def decide(sc):
    """(k, summed scores [COLS]): the antenna sum, the candidates visited 0, -1, +1, ... strictly greater"""
    s = sc.sum(0)
    kbest = 0
    for m in range(1, MAX_RANGE + 1):
        for k in (-m, m):
            if s[k + MAX_RANGE] > s[kbest + MAX_RANGE]:
                kbest = k
    return kbest, s
