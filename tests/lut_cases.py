"""RX windows that exercise every Wiener-LUT profile and a change of the pick inside a packet (TEST
INFRASTRUCTURE, no GPU needed): shared by tests/test_rx_lut_inputs.py (CPU: the inputs do what they
claim, from the oracle alone) and the GPU parity tests of the same windows (tests/test_gpu_parity.py).

The receiver picks the -5 / 15 / 35 dB profile (0 / 1 / 2) nearest to its running SNR estimate after
every DRS operation (rx_synced.cpp:863-891), so the pick changes at 5 dB and at 25 dB. A packet is an
oracle-TX packet through phy_fixtures.channel at a base SNR and, for a noise step, extra AWGN from
sample frac * S of the window to its end at extra_dB relative to the signal power of the window's first
half: the running estimate then falls through a boundary in the middle of the packet.
"""
import functools

import numpy as np

import oracle_py as O
import phy_fixtures as F

SEED = 11
BOUNDARIES_DB = (5.0, 25.0)
CLEARANCE_DB = 2.0

# per packet: (base SNR dB, noise step (frac, extra_dB) or None, expected profiles in order)
_FLAT = [(0.0, None, (0,)), (12.0, None, (1,)), (30.0, None, (2,))]
TABLES = {
    # name: (configuration of phy_fixtures.CONFIGS, packets)
    "C4": ("C4", _FLAT + [(30.0, (0.5, 10.0), (2, 1)), (12.0, (0.5, -8.0), (1, 0))]),
    # SISO zero-forcing under a -8 dB step is ill-conditioned (the oracle's float path leaves its double
    # path by several LSB there), so that packet is not gated at +-1: it is the clamp input below
    "C3": ("C3", _FLAT + [(30.0, (0.5, 10.0), (2, 1))]),
    # |LLR| far past the int16 range on a SISO 256-QAM row
    "C3_clamp": ("C3", [(12.0, (0.5, -8.0), (1, 0))]),
}


def oracle_cfg(table, lr=1, stride=2):
    psd, cfgt = F.CONFIGS[TABLES[table][0]]
    u_max, b_max, _, os_min, L, M = cfgt
    return O.cfg(u_max, b_max, os_min, L, M, lr=lr, stride=stride), O.psdef(*psd)


@functools.lru_cache(maxsize=None)
def windows(table):
    """The table's packets, built once: a list of dicts with the window (complex64 [N_RX, S], read-only),
    the sync report's fields (fine peak, CFO estimate with a small residual error, RMS of antenna 0 for
    packet 0 only), network ID, PLCF type, the transmitted packed bits, the base SNR, the step and the
    expected profiles."""
    name, packets = TABLES[table]
    psd, cfgt = F.CONFIGS[name]
    n_rx, L, M = cfgt[2], cfgt[4], cfgt[5]
    ocf, ops = oracle_cfg(table)
    sz = O.packet_sizes(ops)
    S = O.dims(ocf, ops)["N_packet_os_rs"]
    n_dft_os = O.dims(ocf, ops)["N_b_DFT_os"]
    rng = np.random.default_rng(SEED)
    out = []
    for i, (base, step, expect) in enumerate(packets):
        pcc = O.pack_bits(F.random_bits(rng, 196))
        pdc = O.pack_bits(F.random_bits(rng, sz["G"]))
        nid, pt = 100 + (i % 6), 1 + i % 2
        iq_tx, _ = O.tx(ocf, ops, pcc, pdc, S, network_id=nid, plcf_type=pt)
        off = int(rng.integers(0, 32))
        cfo_dect = rng.uniform(-1.75, 1.75) * 2 * np.pi / n_dft_os  # rad per DECT sample
        H = F.mixing_matrix(rng, n_rx, iq_tx.shape[0])
        win = F.channel(rng, iq_tx, n_rx, S, off, cfo_dect * M / L, base, H=H)
        if step is not None:
            frac, extra_db = step
            p = np.mean(np.abs((H @ iq_tx)[:, : S // 2]) ** 2)  # as phy_fixtures.channel
            sigma = np.sqrt(p / 10 ** (extra_db / 10) / 2)
            s0 = int(frac * S)
            shape = (n_rx, S - s0)
            win = win.astype(np.complex128)
            win[:, s0:] += sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
            win = win.astype(np.complex64)
        est = -cfo_dect + rng.uniform(-0.02, 0.02) * 2 * np.pi / n_dft_os
        win.setflags(write=False)
        out.append(dict(win=win, fine_peak=off, cfo_est=float(np.float32(est)), nid=nid, pt=pt, pcc=pcc, pdc=pdc,
                        sync_rms=[0.123] + [0.0] * 7 if i == 0 else None, base=base, step=step, expect=expect))
    return out


@functools.lru_cache(maxsize=None)
def oracle(table, i, lr=1, stride=2, use_float=False, pick_force=None, pick_stale=False):
    """The oracle's RX of packet i of a table, computed once per argument set (treat as read-only)."""
    ocf, ops = oracle_cfg(table, lr, stride)
    w = windows(table)[i]
    r = O.rx(ocf, ops, w["win"], w["fine_peak"], w["cfo_est"], w["nid"], w["pt"], use_float=use_float,
             sync_rms=w["sync_rms"], pick_force=pick_force, pick_stale=pick_stale)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def check_picks(tag, picks, expect):
    """The pick sequence is the expected pattern (one profile throughout, or a run of the first and then
    a run of the second, each at least twice) and every estimate is CLEARANCE_DB away from both
    boundaries, so that a float / double difference in the estimate cannot flip a pick."""
    prof = [p for p, _ in picks]
    assert len(prof) >= 4, (tag, prof)
    if len(expect) == 1:
        assert prof == [expect[0]] * len(prof), (tag, picks)
    else:
        k = prof.index(expect[1]) if expect[1] in prof else len(prof)
        assert prof == [expect[0]] * k + [expect[1]] * (len(prof) - k), (tag, picks)
        assert k >= 2 and len(prof) - k >= 2, (tag, picks)
    for p, snr in picks:
        for b in BOUNDARIES_DB:
            assert abs(snr - b) >= CLEARANCE_DB, (tag, p, snr, b)
