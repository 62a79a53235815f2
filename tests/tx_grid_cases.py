"""Inputs shared by tests/test_tx_grid_host.py and tests/test_gpu_tx_grid.py (TEST INFRASTRUCTURE): the kernel
forms launch_tx chooses between (kernels/tx.hip; the choice is dev::tx_form_of over the argument block that
host/tx.cpp plan_tx fills), one case per form that TX_CASES of tests/test_gpu_parity.py and the cases of
tests/test_gpu_tx_window.py do not reach. Smallest shapes: u <= 2 and the shortest valid packet of the mode.

A form's signature (what the host file counts):
  ("stream", mode, q8, windowed)            tx_stream_kernel<10, 9, 22, mode, q8, mfma, windowed>
  ("wave" | "block", (L, M, hl), windowed)  tx_kernel_wave / tx_kernel<L, M, hl, windowed>
  ("scratch", windowed)                     tx_big_sym_kernel (+ tx_big_window_kernel) + tx_big_resample_kernel
  ("wave" | "block", "unstaged")            a symbol run's PDC bytes read in place (more than 8192 bytes)
The streaming kernel's third axis, DNRP_TX_MFMA = 0 / 1 / 2, is an environment switch: the GPU files run it.
"""
import numpy as np

import oracle_py as O

STREAM, WAVE, BLOCK, SCRATCH = "stream", "wave", "block", "scratch"
TXS_SISO, TXS_TXDIV, TXS_SM, TXS_TXDIV1, TXS_SM1 = 0, 1, 2, 3, 4
FRACTION = 0.25

# name: (psdef (u, b, PLT, PL, tm, mcs), ctx (u_max, b_max, N_TX_max, os_min, L, M), codebook, bytes by which
#        iq_out lies past a 16-byte boundary, the fields of the form the case is there for)
CASES = {
    # ---- tx_kernel_wave<10, 9, 22>: N_b_DFT_os = 1024 at 10/9 where the streaming kernel declines
    "wave_u1": ((1, 16, 0, 1, 0, 1), (1, 16, 1, 1, 10, 9), 0, 0,            # a 7-pattern STF (u = 1)
                dict(family=WAVE, L=10, M=9, hl=22, staged=1)),
    "wave_misaligned": ((2, 16, 0, 1, 0, 1), (2, 16, 1, 1, 10, 9), 0, 8,    # no 16-byte pair stores
                        dict(family=WAVE, L=10, M=9, hl=22, staged=1)),
    "wave_tm11_64qam": ((2, 16, 0, 2, 11, 5), (2, 16, 8, 1, 10, 9), 0, 0,   # 8 streams: beyond the 4 KiB window,
                        dict(family=WAVE, L=10, M=9, hl=22, staged=0)),     # and beyond 8192 bytes per run
    # ---- the other resampler classes on the wave path
    "wave_os2": ((1, 8, 0, 1, 1, 3), (1, 8, 2, 2, 10, 9), 0, 0, dict(family=WAVE, L=10, M=9, hl=4, staged=1)),
    "wave_40_27": ((1, 16, 0, 1, 0, 1), (1, 16, 1, 1, 40, 27), 0, 0, dict(family=WAVE, L=0, M=0, hl=0, staged=1)),
    # ---- PDC bytes read in place
    "wave_tm6_16qam": ((1, 16, 0, 3, 6, 3), (1, 16, 4, 1, 10, 9), 0, 0, dict(family=WAVE, L=10, M=9, hl=22, staged=0)),
    # (two subslots: the one-subslot packet's runs stay within 8192 bytes)
    "block_tm11_b12": ((1, 12, 0, 2, 11, 5), (1, 12, 8, 1, 10, 9), 0, 0, dict(family=BLOCK, L=10, M=9, hl=22, staged=0)),
    # ---- streaming kernel at (2, 16): W not a permutation (codebook 1), beamforming, 8 spatial streams
    "stream_txdiv_16qam": ((2, 16, 0, 1, 1, 3), (2, 16, 2, 1, 10, 9), 1, 0, dict(family=STREAM, mode=TXS_TXDIV, q8=0)),
    "stream_txdiv_256": ((2, 16, 0, 1, 1, 8), (2, 16, 2, 1, 10, 9), 1, 0, dict(family=STREAM, mode=TXS_TXDIV, q8=1)),
    "stream_txdiv4_256": ((2, 16, 0, 3, 5, 8), (2, 16, 4, 1, 10, 9), 1, 0, dict(family=STREAM, mode=TXS_TXDIV, q8=1)),
    "stream_sm_16qam": ((2, 16, 0, 1, 2, 3), (2, 16, 2, 1, 10, 9), 1, 0, dict(family=STREAM, mode=TXS_SM, q8=0)),
    "stream_sm_256": ((2, 16, 0, 1, 2, 8), (2, 16, 2, 1, 10, 9), 1, 0,
                      dict(family=STREAM, mode=TXS_SM, q8=1, sb_chunks=2)),
    "stream_bf_tm3_16qam": ((2, 16, 0, 1, 3, 3), (2, 16, 2, 1, 10, 9), 3, 0, dict(family=STREAM, mode=TXS_SISO, q8=0)),
    "stream_bf_tm3_256": ((2, 16, 0, 1, 3, 8), (2, 16, 2, 1, 10, 9), 3, 0, dict(family=STREAM, mode=TXS_SISO, q8=1)),
    "stream_bf_tm7_256": ((2, 16, 0, 1, 7, 8), (2, 16, 4, 1, 10, 9), 9, 0, dict(family=STREAM, mode=TXS_SISO, q8=1)),
    "stream_sm8_16qam": ((2, 16, 0, 2, 11, 3), (2, 16, 8, 1, 10, 9), 0, 0,
                         dict(family=STREAM, mode=TXS_SM1, q8=0, sb_chunks=4)),
    # ---- forms TX_CASES reaches at u = 8: here for their windowed instantiations
    "stream_siso_qpsk": ((2, 16, 0, 1, 0, 1), (2, 16, 1, 1, 10, 9), 0, 0, dict(family=STREAM, mode=TXS_SISO, q8=0)),
    "stream_txdiv1_16qam": ((2, 16, 0, 1, 1, 3), (2, 16, 2, 1, 10, 9), 0, 0, dict(family=STREAM, mode=TXS_TXDIV1, q8=0)),
    "stream_sm1_256": ((2, 16, 0, 1, 2, 8), (2, 16, 2, 1, 10, 9), 0, 0, dict(family=STREAM, mode=TXS_SM1, q8=1)),
}
NAMES = list(CASES)
# run with dnrp_ctx_set_tx_windowing(FRACTION) as well
WINDOWED = ["wave_u1", "wave_misaligned", "wave_os2", "wave_40_27", "stream_txdiv_16qam", "stream_txdiv_256",
            "stream_sm_16qam", "stream_sm_256", "stream_siso_qpsk", "stream_txdiv1_16qam", "stream_sm1_256"]
# the Q8 case of each new streaming mode also under DNRP_TX_MFMA = 1 and 2
MFMA = ["stream_txdiv_256", "stream_sm_256", "stream_bf_tm3_256"]
# the cases of tests/test_gpu_tx_window.py: (its CONFIG name, packets, fraction, extra row samples)
OLDER_WINDOWED = [("tm1", 2, 0.25, 0), ("tm1_1_1", 2, 0.25, 0), ("u1_64", 2, 0.25, 0), ("os2_u2b2_tm1", 2, 0.25, 0),
                  ("lm40_27_b12", 2, 0.25, 0), ("C3", 2, 0.25, 0), ("lm1_1_u8b16", 2, 0.25, 0), ("C4", 1, 0.25, 0),
                  ("tm6_u8b16_64qam", 1, 0.25, 0), ("C3", 2, 0.25, 1), ("u2_in_u8b16", 1, 0.25, 0)]

N_PACKETS = 3  # tests/test_gpu_parity.py _tx_parity
N_WINDOWED = 2


def spec5(name):
    """the case in the form of phy_fixtures.TX_ONLY_CASES"""
    psd, ctx, cb, _, _ = CASES[name]
    return (psd, ctx, 1, (), cb)


def signature(form):
    """the signatures (see above) of a dnrp_tx_form dict"""
    fam, w = form["family"], form["windowed"]
    if fam == STREAM:
        return {(STREAM, form["mode"], form["q8"], w)}
    if fam == SCRATCH:
        return {(SCRATCH, w)}
    sig = {(fam, (form["L"], form["M"], form["hl"]), w)}
    if not form["staged"]:
        sig.add((fam, "unstaged"))
    return sig


def host_form(name, windowed=False):
    """the form dnrp_tx_batch takes for a case, from the host-only twin of the choice"""
    import dnrp
    psd, ctx, cb, misalign, _ = CASES[name]
    n = N_WINDOWED if windowed else N_PACKETS
    return dnrp.tx_form_for(ctx, dnrp.psdef(*psd), [cb] * n, out_misalign=misalign,
                            win_fraction=FRACTION if windowed else 0.0)


def windowed_packets(name):
    """bits and descriptors of a case's windowed run: packet 1 with a mixer phase and increment, another
    network ID and PLCF type (the recipe of tests/test_gpu_tx_window.py with the case's codebook)"""
    import dnrp
    import test_gpu_tx_window as W
    psd, ctx, cb, _, _ = CASES[name]
    g = W.geometry(psd, ctx)
    rng = np.random.default_rng(0x717D0 + N_WINDOWED)
    pcc = np.stack([O.pack_bits(rng.integers(0, 2, 196, dtype=np.uint8)) for _ in range(N_WINDOWED)])
    pdc = np.stack([O.pack_bits(rng.integers(0, 2, g["sz"]["G"], dtype=np.uint8)) for _ in range(N_WINDOWED)])
    descs = [dnrp.TxDesc(cb, 100, 1, 5, 1.0, 0.0, 0.0, 0)]
    for i in range(1, N_WINDOWED):
        descs.append(dnrp.TxDesc(cb, 100 + i, 2, 5, 1.0, 0.7 * i, 1.3 * 2 * np.pi / g["Nd"], 0))
    return pcc, pdc, descs, g


def windowed_reference(name, fraction):
    """hw-rate reference of the case's windowed packets (fraction None: no windowing): the oracle's DECT-rate
    streams (ratio 1/1, unmixed), windowed, resampled and mixed by the numpy reference of
    tests/test_gpu_tx_window.py"""
    import test_gpu_tx_window as W
    psd, ctx, cb, _, _ = CASES[name]
    pcc, pdc, descs, g = windowed_packets(name)
    ocf1 = O.cfg(ctx[0], ctx[1], ctx[3], 1, 1)
    out = []
    for i, d in enumerate(descs):
        x, _ = O.tx(ocf1, O.psdef(*psd), pcc[i], pdc[i], g["S1"], codebook=cb, network_id=d.network_id,
                    plcf_type=d.plcf_type)
        x = x[:, :g["total"]]
        out.append(W.resample(x if fraction is None else W.window(x, g, fraction), ctx, g, d.iq_phase_rad,
                              d.iq_phase_increment_s2s_post_resampling_rad))
    return out
