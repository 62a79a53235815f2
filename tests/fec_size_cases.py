"""Inputs shared by tests/test_fec_sizes_host.py and tests/test_gpu_fec_sizes.py (TEST INFRASTRUCTURE):
the turbo code over all 188 code-block sizes K = 40 ... 6144 (csrc/host/fec.cpp kQpp, the per-size
valid lists and start positions, kernels/fec.hip's windows and encoder lane chunks), saturated soft
bits, the false alarm (every code-block CRC24B right, the transport-block CRC24A wrong) and the
transport-block lengths at the block edges of fec_tbcrc_kernel.

numpy, the host calls of dnrp.fec and oracle/fec_np.py only; every input is a pure function of its
arguments, so both files see the same bits and soft bits.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fec_np as ON  # noqa: E402

import dnrp.fec as F  # noqa: E402

Z = 6144
SIZES = ON.cb_sizes()
QMS = (1, 2, 4, 6, 8)
# rate classes as multiples of the circular buffer's 3 (K + 4) valid positions: punctured, exactly
# the buffer, repeated more than twice
RATES = (0.45, 1.0, 2.6)


def qpp_of(K):
    _, f1, f2 = F.cb_size(SIZES.index(K))
    return f1, f2


def grid_G(K, rate, Qm):
    g = int(rate * 3 * (K + 4))
    return g - g % Qm


def size_grid():
    """[(K, rv, rate class, Qm, G)]: every K x rv x rate class as a one-block packet of
    N_TB_bits = K - 24; Qm rotates with the running case number (12 cases per K, 5 orders)"""
    out = []
    for K in SIZES:
        assert ON.cbsegm(K - 24, Z) == (1, [K], 0)
        for rv in range(4):
            for rc, rate in enumerate(RATES):
                Qm = QMS[len(out) % 5]
                out.append((K, rv, rc, Qm, grid_G(K, rate, Qm)))
    return out


def grid_tb(n, K):
    """transport block of grid case n"""
    return np.random.default_rng(1000 + n).integers(0, 256, (K - 24) // 8, dtype=np.uint8)


# C > 1 packets (N_TB_bits, Qm, G, rv) whose G / Qm is no multiple of C: two lengths E, the longer
# blocks start at bit offsets of the d row that are no whole bytes (fec_pack_kernel's splice)
PACK_EXTRAS = [(8184, 1, 12345, 0), (8184, 2, 12346, 1), (8312, 6, 6 * 2101, 2), (40960, 1, 70003, 3),
               (40960, 6, 6 * 10001, 0), (41088, 2, 2 * 30005, 2)]


def cb_E(tbs, Qm, G):
    """rate-matched length of every code block (TS 36.212 5.1.4.1.2, pdc_enc.cpp:196-204)"""
    C, Ks, _ = ON.cbsegm(tbs, Z)
    Gp = G // Qm
    return [Qm * (Gp // C) if r <= C - Gp % C - 1 else Qm * -(-Gp // C) for r in range(C)]


def noisy(bits, snr_db, rng, scale=64.0):
    """BPSK-equivalent soft bits (positive = bit 1, tb2pdc.cpp:173-176) at snr_db, int16"""
    x = 2.0 * bits - 1
    y = x + rng.normal(0, 10 ** (-snr_db / 20), len(bits))
    return np.round(np.clip(y * scale, -32767, 32767)).astype(np.int16)


# ---- the decoder sweep: one packet per K, rv / rate class / SNR class / Qm rotating with the size index
CLEAN, MARGINAL, BELOW = 0, 1, 2
# SNR = 1 / sigma^2 in dB of the +-1 soft bits per rate class: clean, marginal (mostly 3 to 9 iterations),
# just below the decoder's threshold (some blocks fail at 10). The thresholds were read off the host
# decoder: rate class 0 keeps 45 % of the buffer (code rate 0.74; its rv 1 and rv 2 packets carry
# almost no systematic bits and fail at any SNR), class 2 gains 10 log10(2.6) dB over the mother code.
SWEEP_SNR = {0: (30.0, 5.5, 5.0), 1: (30.0, -1.0, -1.5), 2: (30.0, -5.0, -5.5)}


def sweep_case(i):
    """-> (K, rv, rate class, Qm, G, SNR class) of size index i"""
    K = SIZES[i]
    rc, Qm = i % 3, QMS[i % 5]
    return K, i % 4, rc, Qm, grid_G(K, RATES[rc], Qm), (i + i // 12) % 3


def sweep_packet(i, rep=0, snr_class=None):
    """-> (cfg, tb bytes, soft bits) of size index i; rep: another draw of the noise, same TB"""
    K, rv, rc, Qm, G, sc = sweep_case(i)
    sc = sc if snr_class is None else snr_class
    cfg = F.fec_cfg(K - 24, Qm, G, rv=rv)
    tb = np.random.default_rng(5000 + i).integers(0, 256, (K - 24) // 8, dtype=np.uint8)
    d = np.unpackbits(F.pdc_encode(cfg, tb))[:G]
    return cfg, tb, noisy(d, SWEEP_SNR[rc][sc], np.random.default_rng(9000 + 1000 * rep + i))


def numpy_subset():
    """size indices the numpy decoder can afford: every K % 32 != 0 up to 512, the sizes on either side
    of each step change of the table (8 -> 16 at 512, 16 -> 32 at 1024, 32 -> 64 at 2048) and of each
    change of the encoder's lane chunk; the largest sizes are added at the clean SNR by the test"""
    ks = [K for K in SIZES if K <= 512 and K % 32] + [40, 48, 504, 512, 528, 1008, 1024, 1056, 2048, 2112]
    return sorted({SIZES.index(K) for K in ks})


NUMPY_LARGE = (4096, 4160, 6144)


# ---- saturated soft bits
def saturated(bits, flip, rng):
    """+32767 for a 1 and -32768 for a 0, a share `flip` of the signs wrong"""
    b = np.asarray(bits, np.uint8) ^ (rng.random(len(bits)) < flip)
    return np.where(b > 0, 32767, -32768).astype(np.int16)


# (K, Qm, repetition of the 3 (K + 4) buffer, share of flipped signs, rv): per size one share far
# below the host decoder's limit (2 iterations), shares at the limit, one above it (failing at 10)
SAT_CASES = [(40, 1, 15.0, 0.10, 0), (40, 1, 15.0, 0.23, 0), (40, 1, 15.0, 0.28, 1), (40, 1, 15.0, 0.36, 1),
             (96, 2, 2.2, 0.10, 0), (96, 2, 2.2, 0.18, 0), (96, 2, 4.0, 0.24, 2), (96, 2, 4.0, 0.30, 2),
             (512, 4, 3.0, 0.20, 3), (512, 4, 3.0, 0.19, 0), (512, 4, 3.0, 0.26, 0),
             (1056, 6, 2.2, 0.19, 1), (1056, 6, 2.5, 0.19, 0), (1056, 6, 2.5, 0.25, 0),
             (264, 8, 5.0, 0.24, 2), (264, 8, 5.0, 0.23, 3), (264, 8, 5.0, 0.30, 2)]


def sat_packet(n, rv=None, flip=None, draw=0):
    """-> (cfg, tb bytes, soft bits) of SAT_CASES[n]; rv / flip override the case's (HARQ sequence)"""
    K, Qm, rep, fl, rv0 = SAT_CASES[n]
    rv = rv0 if rv is None else rv
    G = grid_G(K, rep, Qm)
    cfg = F.fec_cfg(K - 24, Qm, G, rv=rv)
    tb = np.random.default_rng(300 + n).integers(0, 256, (K - 24) // 8, dtype=np.uint8)
    d = np.unpackbits(F.pdc_encode(cfg, tb))[:G]
    return cfg, tb, saturated(d, fl if flip is None else flip, np.random.default_rng(700 + 10 * n + rv + 100 * draw))


def unclamped_sums(llr, K, rv, w=None):
    """fec_np.rate_dematch's sums without the int16 clamp (int64) -> circular buffer"""
    st, _ = ON._buffer_map(K)
    Ncb = len(st)
    R = Ncb // 96
    k0 = R * (2 * int(np.ceil(Ncb / (8 * R))) * rv + 2)
    valid = np.roll(np.arange(Ncb), -k0)
    valid = valid[st[valid] >= 0]
    w = np.zeros(Ncb, np.int64) if w is None else w.astype(np.int64)
    np.add.at(w, valid[np.arange(len(llr)) % len(valid)], np.asarray(llr, np.int64))
    return w


def np_decode_buffer(w, K):
    """numpy decode of one soft circular buffer of a one-block packet -> (ok, TB bits, iterations)"""
    tbs = K - 24
    ok, bits, it = ON.turbo_decode([w], K, *qpp_of(K), 10,
                                   lambda b: np.array_equal(ON.crc(b[:tbs], ON.CRC24A), b[tbs:]), min_iter=2)[0]
    return bool(ok), bits[:tbs], it


# HARQ sequence of saturated transmissions: (SAT_CASES index, share of flipped signs) over rv 0, 2, 3, 1
HARQ_RVS = (0, 2, 3, 1)
SAT_HARQ = [(0, 0.30), (2, 0.27), (5, 0.25), (6, 0.27), (8, 0.20), (9, 0.22), (11, 0.20), (12, 0.22),
            (14, 0.25), (15, 0.27), (3, 0.40)]


def sat_oneshot():
    """-> [(cfg, tb, soft bits)]: SAT_CASES and the first transmission of every HARQ sequence"""
    return [sat_packet(n) for n in range(len(SAT_CASES))] + \
        [sat_packet(n, rv=HARQ_RVS[0], flip=fl, draw=1) for n, fl in SAT_HARQ]


# ---- the false alarm
def false_alarm_bits(tbs, Qm, G, rv, seed=0):
    """-> (d bits [G], TB bits [tbs]) of a C > 1 transport block whose CRC24A has one bit flipped before
    segmentation, every code block with its correct CRC24B: all code blocks decode, the TB check fails"""
    tb = np.random.default_rng(seed).integers(0, 2, tbs).astype(np.uint8)
    b = np.concatenate([tb, ON.crc(tb, ON.CRC24A)]).astype(np.uint8)
    b[tbs + 11] ^= 1
    C, Ks, Fb = ON.cbsegm(tbs, Z)
    assert C > 1 and Fb == 0
    out, rp = [], 0
    for K, E in zip(Ks, cb_E(tbs, Qm, G)):
        c = b[rp:rp + K - 24]
        c = np.concatenate([c, ON.crc(c, ON.CRC24B)])
        rp += K - 24
        out.append(ON.rate_match(*ON.turbo(c, *qpp_of(K)), E, rv))
    return np.concatenate(out), tb


FALSE_ALARM = (8184, 2, 2 * 8184 + 100, 0)   # tbs (C = 2), Qm, G, rv
CORRECT_MULTI = (8312, 4, 17000, 0)          # a correct C = 2 block
CORRECT_SINGLE = (1000, 2, 2400, 0)          # a correct C = 1 block


def clean_llr(d, amp=40):
    return np.where(np.asarray(d) > 0, amp, -amp).astype(np.int16)


# ---- transport-block CRC edges: byte counts 1023, 15, 0 and 16 mod 1024, all C > 1 with F = 0
TBCRC_BYTES = (1023, 1039, 5120, 5136)


def tbcrc_packet(nbytes, n):
    """-> (cfg, tb bytes, clean soft bits) of a TB of nbytes at rate ~1/2"""
    tbs = 8 * nbytes
    C, Ks, Fb = ON.cbsegm(tbs, Z)
    assert C > 1 and Fb == 0, (nbytes, C, Fb)
    Qm = (2, 4, 6, 8)[n % 4]
    G = 2 * tbs + 240
    G -= G % Qm
    cfg = F.fec_cfg(tbs, Qm, G, rv=n % 4)
    tb = np.random.default_rng(40 + n).integers(0, 256, nbytes, dtype=np.uint8)
    return cfg, tb, clean_llr(np.unpackbits(F.pdc_encode(cfg, tb))[:G])


# ---- continuation with a full second wave: (K, packets) at rate 1/2, 1.0 dB
CONT_SIZES = ((256, 160), (264, 70))
CONT_SNR, CONT_SEED = 1.0, 5


def cont_packets():
    """-> [(cfg, tb, soft bits)], the two sizes interleaved in the batch"""
    rng = np.random.default_rng(CONT_SEED)
    out = []
    for K, n in CONT_SIZES:
        for _ in range(n):
            cfg = F.fec_cfg(K - 24, 2, 2 * K)
            tb = rng.integers(0, 256, (K - 24) // 8, dtype=np.uint8)
            out.append((cfg, tb, noisy(np.unpackbits(F.pdc_encode(cfg, tb))[:2 * K], CONT_SNR, rng)))
    order = np.random.default_rng(CONT_SEED + 1).permutation(len(out))
    return [out[j] for j in order]
