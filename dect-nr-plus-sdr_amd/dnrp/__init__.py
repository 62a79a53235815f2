"""Python host binding of libdnrp.so (include/dnrp.h) — the MI355X DECT NR+ lower PHY.

Mirrors the reference's per-worker PHY objects with batched calls:
  Phy.tx_batch      <- tx_t::generate_tx_packet      (lib/src/phy/tx/tx.cpp:165-314)
  Phy.rx_sync_batch <- sync_chunk_t::search()         (lib/src/phy/rx/sync/sync_chunk.cpp:143-279)
  Phy.rx_pcc_batch  <- rx_synced_t::demoddecod_rx_pcc (rx_synced.cpp:186-323)
  Phy.rx_pdc_batch  <- rx_synced_t::demoddecod_rx_pdc (rx_synced.cpp:325-436)
  Phy.add_network_id <- tx_rx_t::add_new_network_id (tx_rx.hpp:52)
Device buffers are torch tensors on the context's device (torch is plumbing only: allocation
and streams). Errors raise DnrpError carrying the C error code; the library must be present —
there is no fallback path.
"""
import ctypes as C
import os

import numpy as np

# torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7). Loading it
# first lets libdnrp.so bind to the same runtime instead of a second copy from /opt/rocm, so
# device pointers and streams from torch tensors are valid inside the library.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# DNRP_LIB: an alternative build of the library (tools/build_variant.sh, A/B experiments)
LIB_PATH = os.environ.get("DNRP_LIB") or os.path.join(os.path.dirname(_HERE), "libdnrp.so")


class DnrpError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: {code} ({strerror(code)})")
        self.code = code


class Cfg(C.Structure):
    _fields_ = [("u_max", C.c_uint32), ("b_max", C.c_uint32), ("N_TX_max", C.c_uint32), ("os_min", C.c_uint32),
                ("L", C.c_uint32), ("M", C.c_uint32), ("chestim_mode_lr", C.c_uint32),
                ("chestim_lr_stride", C.c_uint32), ("max_batch", C.c_uint32), ("device", C.c_int32)]


class PsDef(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("u", "b", "PacketLengthType", "PacketLength", "tm_mode_index",
                                         "mcs_index", "Z")]


PS_FIELDS = ["N_PACKET_symb", "N_DF_symb", "N_PDC_subc", "N_DRS_subc", "G", "N_PDC_bits", "N_TB_bits", "N_TB_byte",
             "C", "N_samples_STF", "N_samples_STF_CP_only", "N_samples_DF", "N_samples_GI",
             "N_samples_packet_no_GI", "N_samples_packet", "N_bps", "N_eff_TX", "N_SS", "N_TS", "N_TX", "N_b_DFT",
             "N_b_OCC", "N_b_DFT_os", "N_samples_packet_no_GI_os_rs", "N_samples_packet_os_rs"]


class PacketSizes(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in PS_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in PS_FIELDS}


class TxDesc(C.Structure):
    _fields_ = [("codebook_index", C.c_uint32), ("network_id", C.c_uint32), ("plcf_type", C.c_uint32),
                ("GI_percentage", C.c_uint32), ("DAC_scale", C.c_float), ("iq_phase_rad", C.c_float),
                ("iq_phase_increment_s2s_post_resampling_rad", C.c_float), ("optimal_scaling_DAC", C.c_uint32)]


TX_FORM_FIELDS = ["family", "L", "M", "hl", "windowed", "mode", "q8", "mfma", "sb_chunks", "n_seg", "staged", "passes"]
TX_FORM_STREAM, TX_FORM_WAVE, TX_FORM_BLOCK, TX_FORM_SCRATCH = 0, 1, 2, 3
TX_FAMILIES = ("stream", "wave", "block", "scratch")
TXS_SISO, TXS_TXDIV, TXS_SM, TXS_TXDIV1, TXS_SM1 = 0, 1, 2, 3, 4  # dnrp_tx_form.mode of the stream family


class TxForm(C.Structure):
    """dnrp_tx_form: the kernel form of a dnrp_tx_batch (dnrp_tx_last_form, dnrp_tx_form_for)."""
    _fields_ = [(n, C.c_uint32) for n in TX_FORM_FIELDS]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in TX_FORM_FIELDS}
        d["family"] = TX_FAMILIES[d["family"]]
        return d


class SyncReport(C.Structure):
    _fields_ = [("fine_peak_time", C.c_int64), ("cfo_fractional_rad", C.c_float), ("cfo_integer_rad", C.c_float),
                ("u", C.c_uint32), ("b", C.c_uint32), ("N_eff_TX", C.c_uint32), ("window", C.c_uint32),
                ("rms", C.c_float * 8)]

    AUTO_WINDOW = 0xFFFFFFFF

    def __init__(self, fine_peak_time=0, cfo_fractional_rad=0.0, cfo_integer_rad=0.0, u=0, b=0, N_eff_TX=0,
                 window=None, rms=None):
        # window omitted: the report's own index in the batch (one packet per window, resolved by
        # Phy.rx_pcc_batch); rms omitted: no sync RMS, the RX estimates every antenna's
        super().__init__(fine_peak_time, cfo_fractional_rad, cfo_integer_rad, u, b, N_eff_TX,
                         SyncReport.AUTO_WINDOW if window is None else window,
                         (C.c_float * 8)(*(list(rms or []) + [0.0] * 8)[:8]))


class SyncCfg(C.Structure):
    _fields_ = [("u", C.c_uint32), ("b", C.c_uint32), ("N_ant_limited", C.c_uint32), ("chunk_len", C.c_uint32),
                ("max_reports", C.c_uint32)]


class SyncResult(C.Structure):
    _fields_ = [("found", C.c_uint32), ("detection_ant_idx", C.c_uint32), ("detection_rms", C.c_float),
                ("detection_metric", C.c_float), ("detection_time_local", C.c_uint32),
                ("detection_time_with_jump_back_local", C.c_uint32), ("coarse_peak_time_local", C.c_uint32),
                ("fine_peak_time_local", C.c_uint32), ("coarse_peak_time", C.c_int64), ("fine_peak_time", C.c_int64),
                ("coarse_peak_array", C.c_float * 8), ("rms_array", C.c_float * 8), ("cfo_fractional_rad", C.c_float),
                ("cfo_integer_rad", C.c_float), ("u", C.c_uint32), ("b", C.c_uint32), ("N_eff_TX", C.c_uint32),
                ("reserved", C.c_uint32), ("fine_peak_metric", C.c_float * 4), ("fine_peak_index", C.c_uint32 * 4)]


def _np_dtype(st):
    names, formats, offsets = [], [], []
    for name, ct in st._fields_:
        names.append(name)
        if hasattr(ct, "_length_"):
            formats.append((np.dtype(ct._type_), (ct._length_,)))
        else:
            formats.append(np.dtype(ct))
        offsets.append(getattr(st, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": C.sizeof(st)})


SYNC_RESULT_DTYPE = _np_dtype(SyncResult)
SYNC_REPORT_DTYPE = _np_dtype(SyncReport)


def sync_reports(results, windows=None):
    """dnrp_sync_result rows -> dnrp_sync_report array for rx_pcc_batch (vectorised). windows: the
    sync window of each row (default: row i was found in window i)."""
    r = np.zeros(len(results), SYNC_REPORT_DTYPE)
    for k in ("fine_peak_time", "cfo_fractional_rad", "cfo_integer_rad", "u", "b", "N_eff_TX"):
        r[k] = results[k]
    r["rms"] = results["rms_array"]
    r["window"] = np.arange(len(results)) if windows is None else windows
    return r


def found_reports(res, n_found):
    """All packets a sync batch found: res [n_win, max_reports] + n_found [n_win] -> the
    dnrp_sync_report array of the found packets in window order (window = its sync window)."""
    n_found = np.asarray(n_found).astype(np.int64)
    if len(n_found) and (n_found == 1).all():  # one packet per window: a view, no record gather
        return sync_reports(res[:, 0], np.arange(len(n_found)))
    win = np.repeat(np.arange(len(n_found)), n_found)
    # report index within its window: position minus the window's first position (vectorised)
    k = np.arange(len(win), dtype=np.int64) - np.repeat(np.cumsum(n_found) - n_found, n_found)
    return sync_reports(res[win, k], win)


class PccReport(C.Structure):
    _fields_ = [("snr_dB", C.c_float), ("cfo_fractional_rad", C.c_float), ("sto_fractional", C.c_float),
                ("rms", C.c_float * 8)]


class PdcReport(C.Structure):
    _fields_ = [("snr_dB", C.c_float), ("mimo_N_RX", C.c_uint32), ("mimo_N_TS_other", C.c_uint32),
                ("tm_3_7_beamforming_idx", C.c_uint32), ("tm_3_7_beamforming_reciprocal_idx", C.c_uint32)]


MIMO_METRIC_HIGHEST_MIN_RX_POWER, MIMO_METRIC_MAX_RX_POWER, MIMO_METRIC_MIN_SPREAD_RX_POWER = 0, 1, 2
MIMO_MAX_CB = 28  # DNRP_MIMO_MAX_CB
MIMO_NONE = 0xFFFFFFFF


class MimoDetail(C.Structure):
    """dnrp_mimo_detail: the MIMO report's stage, noise variance, candidate scores and the rank / precoder report
    of one PDC request (dnrp_rx_mimo_detail)."""
    _fields_ = [("N_RX", C.c_uint32), ("N_TS", C.c_uint32), ("H", C.c_float * 2 * 4 * 8 * 8), ("nv", C.c_float),
                ("nv_used", C.c_float), ("idx_tx", C.c_uint32), ("idx_rx", C.c_uint32),
                ("score_tx", C.c_float * MIMO_MAX_CB), ("score_rx", C.c_float * MIMO_MAX_CB), ("RI", C.c_uint32),
                ("PMI", C.c_uint32), ("pmi", C.c_uint32 * 3), ("rate", C.c_float * 3),
                ("rate_cb", C.c_float * MIMO_MAX_CB * 3), ("sinr_eff_dB", C.c_float)]


MIMO_DETAIL_DTYPE = np.dtype([("N_RX", np.uint32), ("N_TS", np.uint32), ("H", np.complex64, (8, 8, 4)),
                              ("nv", np.float32), ("nv_used", np.float32), ("idx_tx", np.uint32), ("idx_rx", np.uint32),
                              ("score_tx", np.float32, (MIMO_MAX_CB,)), ("score_rx", np.float32, (MIMO_MAX_CB,)),
                              ("RI", np.uint32), ("PMI", np.uint32), ("pmi", np.uint32, (3,)), ("rate", np.float32, (3,)),
                              ("rate_cb", np.float32, (3, MIMO_MAX_CB)), ("sinr_eff_dB", np.float32)])
assert MIMO_DETAIL_DTYPE.itemsize == C.sizeof(MimoDetail)


class AoaCfg(C.Structure):
    """dnrp_aoa_cfg: antenna positions in carrier wavelengths and the azimuth grid of the Bartlett scan."""
    _fields_ = [("pos", C.c_float * 2 * 8), ("az_min", C.c_float), ("az_max", C.c_float), ("n_grid", C.c_uint32),
                ("reserved", C.c_uint32)]


class AoaReport(C.Structure):
    """dnrp_aoa_report: spatial covariance of the zero-forced DRS pilots and its Bartlett scan (dnrp_rx_aoa)."""
    _fields_ = [("R", C.c_float * 2 * 8 * 8), ("n_cells", C.c_uint32), ("grid_idx", C.c_uint32), ("az_rad", C.c_float),
                ("peak", C.c_float), ("lag_re", C.c_float), ("lag_im", C.c_float), ("reserved", C.c_uint32 * 2)]


AOA_NONE = 0xFFFFFFFF
AOA_REPORT_DTYPE = np.dtype([("R", np.complex64, (8, 8)), ("n_cells", np.uint32), ("grid_idx", np.uint32),
                             ("az_rad", np.float32), ("peak", np.float32), ("lag", np.complex64),
                             ("reserved", np.uint32, (2,))])
assert AOA_REPORT_DTYPE.itemsize == C.sizeof(AoaReport)


def _aoa_cfg(pos, az_min, az_max, n_grid):
    pos = np.asarray(pos, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 2 or not 1 <= pos.shape[0] <= 8:
        raise ValueError("pos: [N_RX <= 8][2] antenna positions (x, y) in wavelengths")
    cfg = AoaCfg()
    for r in range(pos.shape[0]):
        cfg.pos[r][0], cfg.pos[r][1] = float(pos[r, 0]), float(pos[r, 1])
    cfg.az_min, cfg.az_max, cfg.n_grid, cfg.reserved = float(az_min), float(az_max), int(n_grid), 0
    return cfg


class PdcReq(C.Structure):
    """dnrp_pdc_req: PLCF-announced psdef, slot in the preceding PCC batch, network ID, PLCF type."""
    _fields_ = [("psdef", PsDef), ("pcc_index", C.c_uint32), ("network_id", C.c_uint32), ("plcf_type", C.c_uint32)]


class SyncStreamState(C.Structure):
    """dnrp_sync_stream_state: baton_t's uniqueness state across dnrp_rx_sync_stream calls."""
    _fields_ = [("sync_time_last", C.c_int64), ("sync_time_unique_limit", C.c_int64), ("packets", C.c_uint64),
                ("not_unique", C.c_uint64)]


CH_AWGN, CH_FLAT, CH_DOUBLY = 0, 1, 2
CH_NOISELESS_DB = 1000.0
CH_N_SIN = 40  # WIRELESS_CHANNEL_DOUBLY_NOF_SINUSOIDS (link.hpp:126)


class ChannelCfg(C.Structure):
    """dnrp_channel_cfg: simulated wireless channel (simulation/wireless channel_{awgn,flat,doubly})."""
    _fields_ = [("kind", C.c_uint32), ("pdp_idx", C.c_uint32), ("tau_rms_ns", C.c_float), ("fD_Hz", C.c_float),
                ("samp_rate", C.c_uint32), ("large_scale", C.c_float), ("snr_db", C.c_float),
                ("net_bw_norm", C.c_float), ("seed", C.c_uint64)]


class VspaceEmission(C.Structure):
    """dnrp_vspace_emission: one transmission as the receiver's virtual space sees it (vspace.cpp:457-487)."""
    _fields_ = [("t_start", C.c_int64), ("tx_row", C.c_uint32), ("length", C.c_uint32), ("link", C.c_uint32),
                ("own", C.c_uint32), ("gain", C.c_float), ("reserved", C.c_uint32)]


class AdcCfg(C.Structure):
    """dnrp_adc_cfg: the simulated radio's clip_and_quantize (hw_simulator.cpp:710-733)."""
    _fields_ = [("clip_limit", C.c_float), ("n_bits", C.c_uint32)]


class ChscanReq(C.Structure):
    """dnrp_chscan_req: one channel measurement (chscan_t): N_partial scans of `length` samples ending at `end`."""
    _fields_ = [("end", C.c_int64), ("length", C.c_uint32), ("N_partial", C.c_uint32), ("N_ant", C.c_uint32),
                ("reserved", C.c_uint32)]

    def __init__(self, end=0, length=0, N_partial=1, N_ant=0xFFFFFFFF, reserved=0):
        super().__init__(end, length, N_partial, N_ant, reserved)  # N_ant unset: every antenna (chscanner.cpp:43)


EXPORTS = ["dnrp_ctx_create", "dnrp_ctx_destroy", "dnrp_add_network_id", "dnrp_get_packet_sizes",
           "dnrp_compute_packet_sizes", "dnrp_tx_batch", "dnrp_rx_sync_batch",
           "dnrp_rx_pcc_batch", "dnrp_rx_pdc_batch", "dnrp_sync", "dnrp_last_kernel_ms", "dnrp_kernel_time_total",
           "dnrp_strerror", "dnrp_get_radio_device_class", "dnrp_query_param", "dnrp_param_name",
           "dnrp_ring_gather", "dnrp_sync_stream_init", "dnrp_sync_stream_window", "dnrp_rx_sync_stream",
           "dnrp_channel_batch", "dnrp_channel_realization", "dnrp_vspace_mix", "dnrp_chscan_batch",
           "dnrp_tx_transmit_length", "dnrp_tx_packet_json",
           "dnrp_rx_packet_json", "dnrp_crc", "dnrp_fec_cbsegm", "dnrp_fec_cb_size", "dnrp_pcc_encode",
           "dnrp_pcc_decode", "dnrp_pdc_encode", "dnrp_pdc_decode", "dnrp_harq_rx_create", "dnrp_harq_rx_reset",
           "dnrp_harq_rx_destroy", "dnrp_pdc_decode_batch", "dnrp_pdc_encode_batch",
           "dnrp_pcc_decode_batch", "dnrp_pdc_decode_batch_harq", "dnrp_pdc_softbuffer_size",
           "dnrp_pcc_encode_batch", "dnrp_query_table", "dnrp_ctx_set_rx_mode", "dnrp_ctx_set_tx_windowing",
           "dnrp_tx_window", "dnrp_ctx_set_sync_beta_search", "dnrp_ctx_get_sync_beta_search",
           "dnrp_ctx_set_sync_fine_all_antennas", "dnrp_ctx_get_sync_fine_all_antennas", "dnrp_rx_sync_fine_peaks",
           "dnrp_ctx_set_sync_icfo_search", "dnrp_ctx_get_sync_icfo_search", "dnrp_rx_sync_icfo_scores",
           "dnrp_tx_last_form", "dnrp_tx_form_for", "dnrp_ctx_set_rx_sto_tracking", "dnrp_ctx_get_rx_sto_tracking",
           "dnrp_rx_sto_track", "dnrp_ctx_set_rx_mimo_report", "dnrp_ctx_get_rx_mimo_report", "dnrp_rx_mimo_detail",
           "dnrp_ctx_set_rx_cfo_tracking", "dnrp_ctx_get_rx_cfo_tracking", "dnrp_rx_cfo_track",
           "dnrp_ctx_set_rx_aoa", "dnrp_ctx_get_rx_aoa", "dnrp_rx_aoa", "dnrp_aoa_estimate"]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libdnrp.so not built at {LIB_PATH} (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        P = C.c_void_p
        L.dnrp_ctx_create.argtypes = [C.POINTER(Cfg), C.POINTER(P)]
        L.dnrp_ctx_destroy.argtypes = [P]
        L.dnrp_add_network_id.argtypes = [P, C.c_uint32]
        L.dnrp_get_packet_sizes.argtypes = [P, C.POINTER(PsDef), C.POINTER(PacketSizes)]
        L.dnrp_compute_packet_sizes.argtypes = [C.POINTER(Cfg), C.POINTER(PsDef), C.POINTER(PacketSizes)]
        L.dnrp_tx_batch.argtypes = [P, C.POINTER(PsDef), C.c_uint32, C.POINTER(TxDesc), P, P, C.c_uint32, P,
                                    C.c_uint32, P]
        L.dnrp_rx_sync_batch.argtypes = [P, C.POINTER(SyncCfg), C.c_uint32, P, C.c_uint64, C.c_uint64, C.c_uint32,
                                         P, P, P]
        L.dnrp_rx_pcc_batch.argtypes = [P, C.c_uint32, P, P, C.c_uint32, C.c_uint32, P,
                                        C.POINTER(PccReport), P]
        L.dnrp_rx_pdc_batch.argtypes = [P, C.c_uint32, C.POINTER(PdcReq), P, C.c_uint32, C.c_uint32, P, C.c_uint32,
                                        C.POINTER(PdcReport), P]
        L.dnrp_sync.argtypes = [P, P]
        L.dnrp_ctx_set_rx_mode.argtypes = [P, C.c_uint32]
        L.dnrp_ctx_set_tx_windowing.argtypes = [P, C.c_float]
        L.dnrp_tx_window.argtypes = [C.c_uint32, C.c_float, P, C.c_uint32]
        L.dnrp_tx_last_form.argtypes = [P, C.POINTER(TxForm)]
        L.dnrp_tx_form_for.argtypes = [C.POINTER(Cfg), C.POINTER(PsDef), C.c_uint32, P, C.c_uint32, C.c_uint32, C.c_float,
                                       C.POINTER(TxForm)]
        L.dnrp_ctx_set_sync_beta_search.argtypes = [P, C.c_uint32, C.c_float]
        L.dnrp_ctx_get_sync_beta_search.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.dnrp_ctx_set_sync_fine_all_antennas.argtypes = [P, C.c_uint32]
        L.dnrp_ctx_get_sync_fine_all_antennas.argtypes = [P, C.POINTER(C.c_uint32)]
        L.dnrp_rx_sync_fine_peaks.argtypes = [P, C.c_uint32, P, P, P]
        L.dnrp_ctx_set_sync_icfo_search.argtypes = [P, C.c_uint32]
        L.dnrp_ctx_get_sync_icfo_search.argtypes = [P, C.POINTER(C.c_uint32)]
        L.dnrp_rx_sync_icfo_scores.argtypes = [P, C.c_uint32, P, P, P]
        L.dnrp_ctx_set_rx_sto_tracking.argtypes = [P, C.c_uint32, C.c_float]
        L.dnrp_ctx_set_rx_cfo_tracking.argtypes = [P, C.c_uint32, C.c_float]
        L.dnrp_ctx_get_rx_cfo_tracking.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.dnrp_rx_cfo_track.argtypes = [P, C.c_uint32, P, P, C.c_uint32, C.POINTER(C.c_uint32), P]
        L.dnrp_ctx_get_rx_sto_tracking.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.dnrp_rx_sto_track.argtypes = [P, C.c_uint32, P, C.c_uint32, C.POINTER(C.c_uint32), P]
        L.dnrp_ctx_set_rx_mimo_report.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32]
        L.dnrp_ctx_get_rx_mimo_report.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.dnrp_rx_mimo_detail.argtypes = [P, C.c_uint32, P, P]
        L.dnrp_ctx_set_rx_aoa.argtypes = [P, C.POINTER(AoaCfg)]
        L.dnrp_ctx_get_rx_aoa.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(AoaCfg)]
        L.dnrp_rx_aoa.argtypes = [P, C.c_uint32, P, P]
        L.dnrp_aoa_estimate.argtypes = [C.POINTER(AoaCfg), C.c_uint32, P, C.POINTER(AoaReport), P]
        L.dnrp_ring_gather.argtypes = [P, P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, P, C.c_uint32, P, P]
        L.dnrp_channel_batch.argtypes = [P, C.POINTER(ChannelCfg), C.c_uint32, C.c_uint32, P, C.c_uint32, C.c_uint32, P, P,
                                         P, C.c_uint32, P]
        L.dnrp_channel_realization.argtypes = [C.POINTER(ChannelCfg), C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_uint32), P, P, P, P, P]
        L.dnrp_vspace_mix.argtypes = [P, C.POINTER(ChannelCfg), C.POINTER(AdcCfg), C.c_uint32, P, C.c_uint32, P, C.c_uint32,
                                      C.c_uint32, C.c_uint32, P, C.c_uint64, C.c_uint64, C.c_int64, C.c_uint64, P]
        L.dnrp_chscan_batch.argtypes = [P, P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, P, P, P, P, P]
        L.dnrp_tx_transmit_length.argtypes = [C.POINTER(Cfg), C.POINTER(PsDef), C.c_uint32, C.POINTER(C.c_uint32)]
        L.dnrp_tx_packet_json.argtypes = [C.POINTER(Cfg), C.POINTER(PsDef), C.POINTER(TxDesc), C.c_uint32, C.c_uint64,
                                          C.c_int64, P, P, P, C.c_uint32, C.c_char_p]
        L.dnrp_rx_packet_json.argtypes = [C.POINTER(Cfg), C.c_uint32, P, C.c_uint32, C.POINTER(PccReport),
                                          C.POINTER(PdcReport), C.c_char_p]
        L.dnrp_sync_stream_init.argtypes = [P, C.POINTER(SyncCfg), C.POINTER(SyncStreamState)]
        L.dnrp_sync_stream_window.argtypes = [P, C.POINTER(SyncCfg)]
        L.dnrp_sync_stream_window.restype = C.c_uint32
        L.dnrp_rx_sync_stream.argtypes = [P, C.POINTER(SyncCfg), P, C.c_uint64, C.c_uint64, C.c_int64, C.c_uint32,
                                          C.POINTER(SyncStreamState), P, C.POINTER(C.c_uint32), P, P]
        L.dnrp_last_kernel_ms.argtypes = [P, C.c_char_p, C.POINTER(C.c_float)]
        L.dnrp_kernel_time_total.argtypes = [P, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]
        L.dnrp_query_table.argtypes = [C.c_char_p, P, C.c_uint32, P, C.c_uint32]
        L.dnrp_strerror.argtypes = [C.c_int]
        L.dnrp_strerror.restype = C.c_char_p
        _lib = L
    return _lib


def strerror(code):
    return lib().dnrp_strerror(int(code)).decode()


def _chk(rc, what):
    if rc != 0:
        raise DnrpError(rc, what)


def psdef(u, b, plt, pl, tm, mcs, Z=6144):
    return PsDef(u, b, plt, pl, tm, mcs, Z)


def compute_packet_sizes(ps, u_max=None, b_max=None, os_min=1, L=10, M=9):
    """Context-free packet geometry (host only). With u_max/b_max the oversampled fields are set."""
    out = PacketSizes()
    cfg = Cfg(u_max, b_max, 1, os_min, L, M, 1, 2, 1, 0) if u_max else None
    rc = lib().dnrp_compute_packet_sizes(C.byref(cfg) if cfg else None, C.byref(ps), C.byref(out))
    if rc != 0:
        raise DnrpError(rc, "dnrp_compute_packet_sizes")
    return out.as_dict()


def tx_window(N_b_DFT_os, fraction):
    """Host-only: the rising raised-cosine edge of TX OFDM windowing (dnrp_tx_window) for an N_b_DFT_os-point
    symbol at `fraction` as a float32 array of the window length N; the falling edge is its mirror."""
    n = lib().dnrp_tx_window(int(N_b_DFT_os), float(fraction), None, 0)
    if n < 0:
        raise DnrpError(n, f"dnrp_tx_window({N_b_DFT_os}, {fraction})")
    out = np.zeros(n, np.float32)
    _chk(min(0, lib().dnrp_tx_window(int(N_b_DFT_os), float(fraction), C.c_void_p(out.ctypes.data), n)), "dnrp_tx_window")
    return out


def tx_form_for(cfg, ps, codebooks, S=None, out_misalign=0, win_fraction=0.0):
    """Host-only: the kernel form dnrp_tx_batch would take (dnrp_tx_form_for) as a dict. cfg: (u_max, b_max,
    N_TX_max, os_min, L, M); codebooks: one index per packet; S: row length (default: the slot window)."""
    u_max, b_max, ntx, os_min, L, M = cfg
    c = Cfg(u_max, b_max, ntx, os_min, L, M, 1, 2, max(1, len(codebooks)), 0)
    if S is None:
        S = compute_packet_sizes(ps, u_max, b_max, os_min, L, M)["N_samples_packet_os_rs"]
    cb = np.ascontiguousarray(np.asarray(codebooks, dtype=np.uint32))
    out = TxForm()
    _chk(lib().dnrp_tx_form_for(C.byref(c), C.byref(ps), len(cb), C.c_void_p(cb.ctypes.data), int(S), int(out_misalign),
                                float(win_fraction), C.byref(out)), "dnrp_tx_form_for")
    return out.as_dict()


def aoa_estimate(pos, az_min, az_max, n_grid, R, N_RX=None):
    """Host-only: the Bartlett scan of dnrp_aoa_estimate on a covariance R (complex [N_RX, N_RX], or the report's
    [8, 8]; rounded to complex64, as the device stores it) with the code the device scan runs. Returns a dict:
    grid_idx, az_rad, peak, lag (complex) and spectrum float32 [n_grid]."""
    R = np.asarray(R)
    n = int(N_RX) if N_RX is not None else len(np.asarray(pos))
    R8 = np.zeros((8, 8), np.complex64)
    R8[:n, :n] = R[:n, :n]
    cfg, out = _aoa_cfg(pos, az_min, az_max, n_grid), AoaReport()
    spec = np.zeros(max(int(n_grid), 1), np.float32)
    _chk(lib().dnrp_aoa_estimate(C.byref(cfg), n, C.c_void_p(R8.ctypes.data), C.byref(out), C.c_void_p(spec.ctypes.data)),
         "dnrp_aoa_estimate")
    return dict(grid_idx=out.grid_idx, az_rad=out.az_rad, peak=out.peak, lag=complex(out.lag_re, out.lag_im),
                spectrum=spec[:int(n_grid)])


def query_table(name, *args):
    """Host-only: a literal table the library builds its device tables from (dnrp_query_table) as a
    float32 array."""
    a = np.ascontiguousarray(np.asarray(args, dtype=np.uint32))
    ap = C.c_void_p(a.ctypes.data) if len(a) else None
    n = lib().dnrp_query_table(str(name).encode(), ap, len(a), None, 0)
    if n < 0:
        raise DnrpError(n, f"dnrp_query_table({name}, {args})")
    out = np.zeros(max(1, n), np.float32)
    _chk(min(0, lib().dnrp_query_table(str(name).encode(), ap, len(a), C.c_void_p(out.ctypes.data), n)),
         "dnrp_query_table")
    return out[:n]


def sync_icfo_cells(N, b, k):
    """Host-only: the bins, mod N, that candidate k of the integer CFO search sums for a packet of b in an
    N-point transform (dnrp_query_table "sync_icfo_cells"); empty for a candidate that is not searched."""
    return query_table("sync_icfo_cells", N, b, int(k) & 0xFFFFFFFF).astype(np.int64)


def pcc_cells(b, N_TS):
    """Host-only: the 98 PCC cells in mapping order as int rows (l, k) (dnrp_query_table "pcc_cells")."""
    return query_table("pcc_cells", b, N_TS).astype(np.int64).reshape(-1, 2)


def pdc_cells(b, N_TS, N_DF):
    """Host-only: the PDC cells of a packet with N_DF data-field symbols in mapping order as int rows (l, k)
    (dnrp_query_table "pdc_cells")."""
    return query_table("pdc_cells", b, N_TS, N_TS, N_DF).astype(np.int64).reshape(-1, 2)


def symbol_cells(b, N_TS, N_DF):
    """Host-only: int rows (PCC, PDC, DRS cell count) of symbols l = 0..N_DF (dnrp_query_table "symbol_cells")."""
    return query_table("symbol_cells", b, N_TS, N_TS, N_DF).astype(np.int64).reshape(-1, 3)


def drs_cells(b, N_TS, N_DF):
    """Host-only: the DRS symbols of a packet as a list of (l, ts_first, ts_last, k [streams, N_b_OCC/4])
    (dnrp_query_table "drs_cells")."""
    v, nd, out, i = query_table("drs_cells", b, N_TS, N_DF).astype(np.int64), 14 * b, [], 0
    while i < len(v):
        l, first, last = (int(x) for x in v[i:i + 3])
        n = (last - first + 1) * nd
        out.append((l, first, last, v[i + 3:i + 3 + n].reshape(-1, nd)))
        i += 3 + n
    return out


def channel_realization(cfg, window, n_tx, n_rx):
    """Host-only: window `window`'s link realisation of a ChannelCfg (dnrp_channel_realization):
    dict with delay / amp [n_rx, n_tx, taps], period / phase_rev [n_rx, n_tx, taps, 40], coef [n_rx, n_tx]."""
    nt = C.c_uint32()
    _chk(lib().dnrp_channel_realization(C.byref(cfg), window, n_tx, n_rx, C.byref(nt), None, None, None, None, None),
         "dnrp_channel_realization")
    t = max(1, nt.value)
    delay = np.zeros((n_rx, n_tx, t), np.int32)
    amp = np.zeros((n_rx, n_tx, t), np.float32)
    period = np.zeros((n_rx, n_tx, t, CH_N_SIN), np.int64)
    phase = np.zeros((n_rx, n_tx, t, CH_N_SIN), np.float64)
    coef = np.zeros((n_rx, n_tx, 2), np.float32)
    _chk(lib().dnrp_channel_realization(C.byref(cfg), window, n_tx, n_rx, C.byref(nt), C.c_void_p(delay.ctypes.data),
                                        C.c_void_p(amp.ctypes.data), C.c_void_p(period.ctypes.data),
                                        C.c_void_p(phase.ctypes.data), C.c_void_p(coef.ctypes.data)),
         "dnrp_channel_realization")
    k = nt.value
    return {"delay": delay[..., :k], "amp": amp[..., :k], "period": period[:, :, :k], "phase_rev": phase[:, :, :k],
            "coef": coef[..., 0] + 1j * coef[..., 1]}


def _host_cfg(u_max, b_max, n_ant, os_min=1, L=10, M=9):
    return Cfg(u_max, b_max, n_ant, os_min, L, M, 1, 2, 1, 0)


def tx_transmit_length(ps, GI_percentage, u_max, b_max, os_min=1, L=10, M=9):
    """Host-only: N_samples_transmit_os_rs (tx.cpp:555-566) of a packet configuration."""
    out = C.c_uint32()
    _chk(lib().dnrp_tx_transmit_length(C.byref(_host_cfg(u_max, b_max, 1, os_min, L, M)), C.byref(ps), GI_percentage,
                                       C.byref(out)), "dnrp_tx_transmit_length")
    return int(out.value)


def tx_packet_json(path, ps, desc, pcc_d, pdc_d, iq, u_max, b_max, n_tx, os_min=1, L=10, M=9, rv=0, tx_order_id=0,
                   tx_time_64=0):
    """Host-only: tx_t::write_all_data_to_json of one packet. pcc_d / pdc_d uint8 (packed d-bits),
    iq complex64 [N_TX, S] (a host copy of the dnrp_tx_batch output row)."""
    pcc = np.ascontiguousarray(pcc_d, np.uint8)
    pdc = np.ascontiguousarray(pdc_d, np.uint8)
    x = np.ascontiguousarray(iq, np.complex64)
    _chk(lib().dnrp_tx_packet_json(C.byref(_host_cfg(u_max, b_max, n_tx, os_min, L, M)), C.byref(ps), C.byref(desc), rv,
                                   tx_order_id, tx_time_64, C.c_void_p(pcc.ctypes.data), C.c_void_p(pdc.ctypes.data),
                                   C.c_void_p(x.ctypes.data), x.shape[1], str(path).encode()), "dnrp_tx_packet_json")


def rx_packet_json(path, sync_result, u_max, b_max, n_ant, mcs_index, pcc_report=None, pdc_report=None, os_min=1, L=10,
                   M=9, worker_id=0):
    """Host-only: the RADIO/PHY part of worker_tx_rx_t::collect_and_write_json for one packet."""
    r = np.ascontiguousarray(np.asarray(sync_result, dtype=SYNC_RESULT_DTYPE).reshape(1))
    _chk(lib().dnrp_rx_packet_json(C.byref(_host_cfg(u_max, b_max, n_ant, os_min, L, M)), worker_id,
                                   C.c_void_p(r.ctypes.data), mcs_index, C.byref(pcc_report) if pcc_report else None,
                                   C.byref(pdc_report) if pdc_report else None, str(path).encode()),
         "dnrp_rx_packet_json")


def _check_tensor(t, what, dtype, ndim, device):
    """Shapes, dtype, layout and device of a buffer handed to libdnrp.so (the C side trusts them)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{what}: {t.dim()} dimensions, expected {ndim}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    if t.device.type != "cuda" or (t.device.index or 0) != device:
        raise ValueError(f"{what}: must live on cuda:{device}, is on {t.device}")


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream))


class Phy:
    """One context = one submitting thread (like one worker_tx_rx_t)."""

    def __init__(self, u_max, b_max, N_TX_max, os_min=1, L=10, M=9, chestim_mode_lr=True, stride=2, max_batch=64,
                 device=0):
        self.cfg = Cfg(u_max, b_max, N_TX_max, os_min, L, M, int(chestim_mode_lr), stride, max_batch, device)
        self._ctx = C.c_void_p()
        _chk(lib().dnrp_ctx_create(C.byref(self.cfg), C.byref(self._ctx)), "dnrp_ctx_create")

    def close(self):
        if self._ctx:
            lib().dnrp_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    RX_MODE_SM_MMSE = 1

    def set_rx_mode(self, flags):
        """dnrp_ctx_set_rx_mode: RX_MODE_SM_MMSE enables the MMSE receiver for spatial multiplexing."""
        _chk(lib().dnrp_ctx_set_rx_mode(self._ctx, int(flags)), "dnrp_ctx_set_rx_mode")

    def set_tx_windowing(self, fraction):
        """dnrp_ctx_set_tx_windowing: raised-cosine symbol transitions (the reference's build option
        PHY_TX_OFDM_WINDOWING) for every later tx_batch; 0 turns them off (the default)."""
        _chk(lib().dnrp_ctx_set_tx_windowing(self._ctx, float(fraction)), "dnrp_ctx_set_tx_windowing")

    def tx_last_form(self):
        """dnrp_tx_last_form: the kernel form of the latest tx_batch as a dict (family "stream" / "wave" / "block" /
        "scratch", resampler class, windowed, and the family's fields)."""
        out = TxForm()
        _chk(lib().dnrp_tx_last_form(self._ctx, C.byref(out)), "dnrp_tx_last_form")
        return out.as_dict()

    def set_sync_beta_search(self, on, threshold_db=-10.0):
        """dnrp_ctx_set_sync_beta_search: every later rx_sync_batch / rx_sync_stream estimates the packet's
        b at the coarse peak (the reference's build option
        RX_SYNC_PARAM_AUTOCORRELATOR_PEAK_FIND_BETA_THRESHOLD_DB_OR_ASSUME_MAX_OF_RDC) and cross-correlates
        against the templates of that b; off (the default) reports b = SyncCfg.b."""
        _chk(lib().dnrp_ctx_set_sync_beta_search(self._ctx, int(on), float(threshold_db)), "dnrp_ctx_set_sync_beta_search")

    def sync_beta_search(self):
        """dnrp_ctx_get_sync_beta_search: (on, threshold_db, threshold_linear = 10 ** (dB / 20))."""
        on, db, lin = C.c_uint32(), C.c_float(), C.c_float()
        _chk(lib().dnrp_ctx_get_sync_beta_search(self._ctx, C.byref(on), C.byref(db), C.byref(lin)),
             "dnrp_ctx_get_sync_beta_search")
        return bool(on.value), db.value, lin.value

    def set_sync_fine_all_antennas(self, on):
        """dnrp_ctx_set_sync_fine_all_antennas: every later rx_sync_batch / rx_sync_stream cross-correlates every
        searched antenna that has a coarse peak against the STF templates and combines the peaks by their
        metrics (the reference's build option RX_SYNC_PARAM_CROSSCORRELATOR_ALL_ANTENNAS_OR_ONLY_STRONGEST);
        off (the default) searches the strongest antenna only."""
        _chk(lib().dnrp_ctx_set_sync_fine_all_antennas(self._ctx, int(on)), "dnrp_ctx_set_sync_fine_all_antennas")

    def sync_fine_all_antennas(self):
        """dnrp_ctx_get_sync_fine_all_antennas"""
        on = C.c_uint32()
        _chk(lib().dnrp_ctx_get_sync_fine_all_antennas(self._ctx, C.byref(on)), "dnrp_ctx_get_sync_fine_all_antennas")
        return bool(on.value)

    def set_sync_icfo_search(self, search_range):
        """dnrp_ctx_set_sync_icfo_search: every later rx_sync_batch / rx_sync_stream searches the integer CFO
        k in [-search_range, search_range] (multiples of 4 subcarriers) at the coarse peak and reports
        cfo_integer_rad = -k 8 pi / N; 0 (the default) = off, the synchronisation as it is without the search."""
        _chk(lib().dnrp_ctx_set_sync_icfo_search(self._ctx, int(search_range)), "dnrp_ctx_set_sync_icfo_search")

    def sync_icfo_search(self):
        """dnrp_ctx_get_sync_icfo_search: the range, 0 = off"""
        r = C.c_uint32()
        _chk(lib().dnrp_ctx_get_sync_icfo_search(self._ctx, C.byref(r)), "dnrp_ctx_get_sync_icfo_search")
        return int(r.value)

    def sync_icfo_scores(self, n_reports, stream=None):
        """dnrp_rx_sync_icfo_scores: (score float32 [n_reports, 8, 9] = (report slot of the latest rx_sync_batch,
        antenna, candidate k + 4), k int32 [n_reports]); -1 where a candidate is outside the range or not
        searched. n_reports = n * max_reports of that call, which ran with set_sync_icfo_search(1..4)."""
        score = np.zeros((int(n_reports), 8, 9), np.float32)
        k = np.zeros(int(n_reports), np.int32)
        _chk(lib().dnrp_rx_sync_icfo_scores(self._ctx, int(n_reports), C.c_void_p(score.ctypes.data),
                                            C.c_void_p(k.ctypes.data), _stream_ptr(stream)), "dnrp_rx_sync_icfo_scores")
        return score, k

    def sync_fine_peaks(self, n_reports, stream=None):
        """dnrp_rx_sync_fine_peaks: (metric float32, index uint32), each [n_reports, 8, 4] = (report slot of the
        latest rx_sync_batch in res order, antenna, template), 0 where not processed; n_reports = n * max_reports
        of that call, which ran with set_sync_fine_all_antennas(1). Synchronises the stream before it returns."""
        metric = np.zeros((n_reports, 8, 4), np.float32)
        index = np.zeros((n_reports, 8, 4), np.uint32)
        _chk(lib().dnrp_rx_sync_fine_peaks(self._ctx, int(n_reports), C.c_void_p(metric.ctypes.data),
                                           C.c_void_p(index.ctypes.data), _stream_ptr(stream)), "dnrp_rx_sync_fine_peaks")
        self.sync(stream)
        return metric, index

    def set_rx_sto_tracking(self, on, gain=1.0):
        """dnrp_ctx_set_rx_sto_tracking: every later rx_pcc_batch (and its rx_pdc_batch) adds, after each DRS
        symbol, gain times the slope of its zero-forced pilots over frequency to the STO increment the later
        symbols are derotated with (the reference's build option RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS);
        off (the default) derotates every symbol with the STF estimate."""
        _chk(lib().dnrp_ctx_set_rx_sto_tracking(self._ctx, int(on), float(gain)), "dnrp_ctx_set_rx_sto_tracking")

    def rx_sto_tracking(self):
        """dnrp_ctx_get_rx_sto_tracking: (on, gain)."""
        on, gain = C.c_uint32(), C.c_float()
        _chk(lib().dnrp_ctx_get_rx_sto_tracking(self._ctx, C.byref(on), C.byref(gain)), "dnrp_ctx_get_rx_sto_tracking")
        return bool(on.value), gain.value

    def rx_sto_track(self, n_slots, stream=None):
        """dnrp_rx_sto_track: float64 [n_slots, n_sym], the STO increment each OFDM symbol of the first n_slots
        PCC-batch slots was derotated with by the latest rx_pcc_batch / rx_pdc_batch, which ran with
        set_rx_sto_tracking(1): symbol 0 the STF estimate, NaN where a symbol was not processed. Synchronises
        the stream before it returns."""
        n_sym = C.c_uint32()
        _chk(lib().dnrp_rx_sto_track(self._ctx, int(n_slots), None, 0, C.byref(n_sym), _stream_ptr(stream)),
             "dnrp_rx_sto_track")
        inc = np.full((int(n_slots), n_sym.value), np.nan, np.float64)
        _chk(lib().dnrp_rx_sto_track(self._ctx, int(n_slots), C.c_void_p(inc.ctypes.data), n_sym.value, C.byref(n_sym),
                                     _stream_ptr(stream)), "dnrp_rx_sto_track")
        self.sync(stream)
        return inc

    def set_rx_mimo_report(self, metric=0, all_w=0, detail=0):
        """dnrp_ctx_set_rx_mimo_report: every later rx_pdc_batch searches the single-stream codebooks with
        `metric` (MIMO_METRIC_*, the reference's build option RX_SYNCED_PARAM_MODE_3_7_METRIC) from entry 0
        (all_w = 1, RX_SYNCED_PARAM_MIMO_USE_ALL_W_MATRICES_OR_ONLY_NON_ZERO) or from the first entry without a
        zero; detail = 1 keeps one dnrp_mimo_detail row per request (rx_mimo_detail). (0, 0, 0), the default, is
        the reference's default build."""
        _chk(lib().dnrp_ctx_set_rx_mimo_report(self._ctx, int(metric), int(all_w), int(detail)),
             "dnrp_ctx_set_rx_mimo_report")

    def rx_mimo_report(self):
        """dnrp_ctx_get_rx_mimo_report: (metric, all_w, detail)."""
        me, aw, de = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(lib().dnrp_ctx_get_rx_mimo_report(self._ctx, C.byref(me), C.byref(aw), C.byref(de)),
             "dnrp_ctx_get_rx_mimo_report")
        return me.value, aw.value, de.value

    def rx_mimo_detail(self, m, stream=None):
        """dnrp_rx_mimo_detail: numpy record array [m] of MIMO_DETAIL_DTYPE (fields are views: H complex64
        [m, 8, 8, 4], score_tx / score_rx [m, 28], rate_cb [m, 3, 28], ...), row r = request r of the latest
        rx_pdc_batch, which ran with set_rx_mimo_report(detail=1). Synchronises the stream before it returns."""
        out = np.zeros(int(m), MIMO_DETAIL_DTYPE)
        _chk(lib().dnrp_rx_mimo_detail(self._ctx, int(m), C.c_void_p(out.ctypes.data) if m else None, _stream_ptr(stream)),
             "dnrp_rx_mimo_detail")
        self.sync(stream)
        return out

    def set_rx_aoa(self, pos, az_min=-np.pi / 2, az_max=np.pi / 2, n_grid=181):
        """dnrp_ctx_set_rx_aoa: every later rx_pdc_batch reports, per request, the spatial covariance of the
        zero-forced DRS pilots and its Bartlett scan over n_grid azimuths in [az_min, az_max] (cyclic where the
        span is 2 pi) for antennas at pos [N_RX][2] (x, y) in carrier wavelengths (rx_aoa). set_rx_aoa(None), the
        default, turns it off."""
        if pos is None:
            _chk(lib().dnrp_ctx_set_rx_aoa(self._ctx, None), "dnrp_ctx_set_rx_aoa")
            return
        cfg = _aoa_cfg(pos, az_min, az_max, n_grid)
        _chk(lib().dnrp_ctx_set_rx_aoa(self._ctx, C.byref(cfg)), "dnrp_ctx_set_rx_aoa")

    def rx_aoa_cfg(self):
        """dnrp_ctx_get_rx_aoa: None while off, else (pos float32 [8, 2], az_min, az_max, n_grid)."""
        on, cfg = C.c_uint32(), AoaCfg()
        _chk(lib().dnrp_ctx_get_rx_aoa(self._ctx, C.byref(on), C.byref(cfg)), "dnrp_ctx_get_rx_aoa")
        if not on.value:
            return None
        return np.ctypeslib.as_array(cfg.pos).astype(np.float32).reshape(8, 2), cfg.az_min, cfg.az_max, cfg.n_grid

    def rx_aoa(self, m, stream=None):
        """dnrp_rx_aoa: numpy record array [m] of AOA_REPORT_DTYPE (R complex64 [m, 8, 8], lag complex64, ...),
        row r = request r of the latest rx_pdc_batch, which ran with set_rx_aoa on. Synchronises the stream
        before it returns."""
        out = np.zeros(int(m), AOA_REPORT_DTYPE)
        _chk(lib().dnrp_rx_aoa(self._ctx, int(m), C.c_void_p(out.ctypes.data) if m else None, _stream_ptr(stream)),
             "dnrp_rx_aoa")
        self.sync(stream)
        return out

    def set_rx_cfo_tracking(self, on, gain=1.0):
        """dnrp_ctx_set_rx_cfo_tracking: every later rx_pcc_batch (and its rx_pdc_batch) takes, after each DRS
        symbol that has an earlier one of the same transmit streams, gain times the rotation between the two per
        sample off the mixer increment of the later symbols (the intent of the reference's build option
        RX_SYNCED_PARAM_CFO_RESIDUAL_BASED_ON_DRS); off (the default) mixes every symbol with the STF's increment."""
        _chk(lib().dnrp_ctx_set_rx_cfo_tracking(self._ctx, int(on), float(gain)), "dnrp_ctx_set_rx_cfo_tracking")

    def rx_cfo_tracking(self):
        """dnrp_ctx_get_rx_cfo_tracking: (on, gain)."""
        on, gain = C.c_uint32(), C.c_float()
        _chk(lib().dnrp_ctx_get_rx_cfo_tracking(self._ctx, C.byref(on), C.byref(gain)), "dnrp_ctx_get_rx_cfo_tracking")
        return bool(on.value), gain.value

    def rx_cfo_track(self, n_slots, stream=None):
        """dnrp_rx_cfo_track: float64 [n_slots, n_sym, 2], the mixer entry (phase a, increment) each OFDM symbol of
        the first n_slots PCC-batch slots was mixed with by the latest rx_pcc_batch / rx_pdc_batch, which ran with
        set_rx_cfo_tracking(1): DECT-rate sample m of symbol l got the phase a + (m - n_stf) inc. NaN where a
        symbol was not processed. Synchronises the stream before it returns."""
        n_sym = C.c_uint32()
        _chk(lib().dnrp_rx_cfo_track(self._ctx, int(n_slots), None, None, 0, C.byref(n_sym), _stream_ptr(stream)),
             "dnrp_rx_cfo_track")
        inc = np.full((int(n_slots), n_sym.value), np.nan, np.float64)
        phase = np.full((int(n_slots), n_sym.value), np.nan, np.float64)
        _chk(lib().dnrp_rx_cfo_track(self._ctx, int(n_slots), C.c_void_p(inc.ctypes.data), C.c_void_p(phase.ctypes.data),
                                     n_sym.value, C.byref(n_sym), _stream_ptr(stream)), "dnrp_rx_cfo_track")
        self.sync(stream)
        return np.stack([phase, inc], axis=2)

    def add_network_id(self, nid):
        _chk(lib().dnrp_add_network_id(self._ctx, nid), "dnrp_add_network_id")

    def packet_sizes(self, ps):
        out = PacketSizes()
        _chk(lib().dnrp_get_packet_sizes(self._ctx, C.byref(ps), C.byref(out)), "dnrp_get_packet_sizes")
        return out.as_dict()

    def tx_batch(self, ps, descs, pcc_d, pdc_d, iq_out, stream=None):
        """pcc_d uint8 [n,25], pdc_d uint8 [n,stride], iq_out float32 [n,N_TX,S,2] (torch, device)."""
        import torch
        n = len(descs)
        dev = int(self.cfg.device)
        _check_tensor(pcc_d, "pcc_d", torch.uint8, 2, dev)
        _check_tensor(pdc_d, "pdc_d", torch.uint8, 2, dev)
        _check_tensor(iq_out, "iq_out", torch.float32, 4, dev)
        sz = self.packet_sizes(ps)
        if pcc_d.shape[0] < n or pcc_d.shape[1] != 25:
            raise ValueError(f"pcc_d shape {tuple(pcc_d.shape)}, expected [>={n}, 25]")
        if pdc_d.shape[0] < n or pdc_d.shape[1] < (sz["G"] + 7) // 8:
            raise ValueError(f"pdc_d shape {tuple(pdc_d.shape)}, expected [>={n}, >={(sz['G'] + 7) // 8}]")
        if iq_out.shape[0] < n or iq_out.shape[1] != sz["N_TX"] or iq_out.shape[3] != 2:
            raise ValueError(f"iq_out shape {tuple(iq_out.shape)}, expected [>={n}, {sz['N_TX']}, S, 2]")
        arr = descs if isinstance(descs, C.Array) else (TxDesc * n)(*descs)
        _chk(lib().dnrp_tx_batch(self._ctx, C.byref(ps), n, arr, C.c_void_p(pcc_d.data_ptr()),
                                 C.c_void_p(pdc_d.data_ptr()), pdc_d.shape[1], C.c_void_p(iq_out.data_ptr()),
                                 iq_out.shape[2], _stream_ptr(stream)), "dnrp_tx_batch")

    def rx_sync_batch(self, sc, iq, n, S_win, win_stride, ant_stride, res=None, n_found=None, stream=None):
        """sync_chunk_t::search() on n windows of the device cf32 tensor iq (strides in samples).
        res: numpy SYNC_RESULT_DTYPE [n, max_reports] (pinned memory keeps the copy asynchronous);
        valid after sync(). Returns (res, n_found)."""
        import torch
        _check_tensor(iq, "iq", torch.float32, iq.dim(), int(self.cfg.device))
        if iq.shape[-1] != 2:
            raise ValueError("iq: last dimension must be 2 (interleaved cf32)")
        if n > 0:
            last = (n - 1) * win_stride + (sc.N_ant_limited - 1) * ant_stride + S_win
            if last > iq.numel() // 2:
                raise ValueError(f"iq holds {iq.numel() // 2} samples, the windows reach {last}")
        if res is None:
            res = np.zeros((n, sc.max_reports), SYNC_RESULT_DTYPE)
        if n_found is None:
            n_found = np.zeros(n, np.uint32)
        assert res.dtype == SYNC_RESULT_DTYPE and res.size >= n * sc.max_reports and res.flags.c_contiguous
        assert n_found.dtype == np.uint32 and n_found.size >= n
        _chk(lib().dnrp_rx_sync_batch(self._ctx, C.byref(sc), n, C.c_void_p(iq.data_ptr()), win_stride, ant_stride,
                                      S_win, C.c_void_p(res.ctypes.data), C.c_void_p(n_found.ctypes.data),
                                      _stream_ptr(stream)), "dnrp_rx_sync_batch")
        return res, n_found

    def _check_rx_windows(self, iq_in):
        import torch
        _check_tensor(iq_in, "iq_in", torch.float32, 4, int(self.cfg.device))
        if iq_in.shape[1] != self.cfg.N_TX_max or iq_in.shape[3] != 2:
            raise ValueError(f"iq_in shape {tuple(iq_in.shape)}, expected [windows, {self.cfg.N_TX_max}, S_in, 2]")

    def rx_pcc_batch(self, reports, iq_in, pcc_llr, want_report=False, stream=None):
        """reports: list of SyncReport or a numpy SYNC_REPORT_DTYPE array (see sync_reports()).
        iq_in float32 [n, N_RX, S_in, 2]; pcc_llr int16 [n, 196]."""
        import torch
        n = len(reports)
        self._check_rx_windows(iq_in)
        _check_tensor(pcc_llr, "pcc_llr", torch.int16, 2, int(self.cfg.device))
        if pcc_llr.shape[0] < n or pcc_llr.shape[1] != 196:
            raise ValueError(f"pcc_llr shape {tuple(pcc_llr.shape)}, expected [>={n}, 196]")
        if isinstance(reports, np.ndarray):
            assert reports.dtype == SYNC_REPORT_DTYPE and reports.flags.c_contiguous
            wins = reports["window"]
            arr = C.c_void_p(reports.ctypes.data)
        else:
            arr_s = (SyncReport * n)(*reports)
            for i in range(n):  # SyncReport(...) without a window: its own index
                if arr_s[i].window == SyncReport.AUTO_WINDOW:
                    arr_s[i].window = i
            wins = np.array([r.window for r in arr_s], np.int64)
            arr = C.cast(arr_s, C.c_void_p)
        if n and (wins.max() >= iq_in.shape[0] or wins.min() < 0):
            raise ValueError(f"sync report window {int(wins.max())} outside iq_in ({iq_in.shape[0]} windows)")
        rep = (PccReport * n)() if want_report else None
        _chk(lib().dnrp_rx_pcc_batch(self._ctx, n, arr, C.c_void_p(iq_in.data_ptr()), iq_in.shape[0], iq_in.shape[2],
                                     C.c_void_p(pcc_llr.data_ptr()), rep, _stream_ptr(stream)), "dnrp_rx_pcc_batch")
        return rep

    def rx_pdc_batch(self, reqs, iq_in, pdc_llr, want_report=False, stream=None):
        """reqs: PdcReq per packet the MAC continues with (psdef, pcc_index, network_id, plcf_type);
        iq_in: the windows of the preceding rx_pcc_batch; pdc_llr int16 [m, >= max G] (row r = reqs[r])."""
        import torch
        m = len(reqs)
        self._check_rx_windows(iq_in)
        _check_tensor(pdc_llr, "pdc_llr", torch.int16, 2, int(self.cfg.device))
        arr = reqs if isinstance(reqs, C.Array) else (PdcReq * m)(*reqs)
        # distinct psdefs of the requests, vectorised over the array's memory (a Python loop over
        # 16384 ctypes records takes ~50 ms per call)
        nw = C.sizeof(PsDef) // 4  # PsDef: uint32 fields only
        w = np.frombuffer(arr, dtype=np.uint32, count=m * C.sizeof(PdcReq) // 4).reshape(m, -1)[:, :nw] if m else None
        if w is None:
            keys = set()
        elif (w == w[0]).all():
            keys = {tuple(int(x) for x in w[0])}
        else:
            rows = np.unique(np.ascontiguousarray(w).view(np.dtype((np.void, 4 * nw))).ravel())
            keys = {tuple(int(x) for x in np.frombuffer(r.tobytes(), np.uint32)) for r in rows}
        g_max = max((self.packet_sizes(PsDef(*k))["G"] for k in keys), default=0)
        if pdc_llr.shape[0] < m or pdc_llr.shape[1] < g_max:
            raise ValueError(f"pdc_llr shape {tuple(pdc_llr.shape)}, expected [>={m}, >={g_max}]")
        rep = (PdcReport * m)() if want_report else None
        _chk(lib().dnrp_rx_pdc_batch(self._ctx, m, arr, C.c_void_p(iq_in.data_ptr()), iq_in.shape[0], iq_in.shape[2],
                                     C.c_void_p(pdc_llr.data_ptr()), pdc_llr.shape[1], rep, _stream_ptr(stream)),
             "dnrp_rx_pdc_batch")
        return rep

    def sync(self, stream=None):
        _chk(lib().dnrp_sync(self._ctx, _stream_ptr(stream)), "dnrp_sync")

    def _check_ring(self, ring, n_ant):
        import torch
        _check_tensor(ring, "ring", torch.float32, 3, int(self.cfg.device))
        if ring.shape[0] < n_ant or ring.shape[2] != 2:
            raise ValueError(f"ring shape {tuple(ring.shape)}, expected [>= {n_ant}, ring_len, 2]")

    def ring_gather(self, ring, starts, S_win, out, n_ant=None, stream=None):
        """buffer_rx_t ring (float32 [N_ant, ring_len, 2], sample t at t % ring_len) -> windows
        out float32 [n, n_ant, S_win, 2] starting at the global times `starts` (rx_pacer wrap copy)."""
        import torch
        n_ant = n_ant or ring.shape[0]
        self._check_ring(ring, n_ant)
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int64))
        n = len(st)
        _check_tensor(out, "out", torch.float32, 4, int(self.cfg.device))
        if out.shape[0] < n or out.shape[1] != n_ant or out.shape[2] != S_win or out.shape[3] != 2:
            raise ValueError(f"out shape {tuple(out.shape)}, expected [>={n}, {n_ant}, {S_win}, 2]")
        _chk(lib().dnrp_ring_gather(self._ctx, C.c_void_p(ring.data_ptr()), ring.shape[1], ring.shape[1], n_ant, n,
                                    C.c_void_p(st.ctypes.data), S_win, C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
             "dnrp_ring_gather")

    def channel_batch(self, cfg, tx, offsets, t0s, rx, stream=None):
        """Simulated channel: tx float32 [n, N_TX, S_tx, 2] -> rx float32 [n, N_RX, S_rx, 2] (device);
        offsets / t0s: per window, TX sample 0 at RX sample offset, global time of RX sample 0."""
        import torch
        dev = int(self.cfg.device)
        _check_tensor(tx, "tx", torch.float32, 4, dev)
        _check_tensor(rx, "rx", torch.float32, 4, dev)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        t0 = np.ascontiguousarray(np.asarray(t0s, dtype=np.int64))
        n = len(off)
        if len(t0) != n or tx.shape[0] < n or rx.shape[0] < n or tx.shape[3] != 2 or rx.shape[3] != 2:
            raise ValueError("channel_batch: window counts / shapes disagree")
        _chk(lib().dnrp_channel_batch(self._ctx, C.byref(cfg), n, tx.shape[1], C.c_void_p(tx.data_ptr()), tx.shape[2],
                                      rx.shape[1], C.c_void_p(off.ctypes.data), C.c_void_p(t0.ctypes.data),
                                      C.c_void_p(rx.data_ptr()), rx.shape[2], _stream_ptr(stream)), "dnrp_channel_batch")

    def vspace_mix(self, cfg, emissions, tx, ring, t_begin, n_samples, adc=None, stream=None, ring_len=None):
        """Virtual space (dnrp_vspace_mix): the emissions (VspaceEmission list or array), their samples in
        tx float32 [n_rows, N_TX, S_tx, 2], through the links of ChannelCfg `cfg` into global samples
        [t_begin, t_begin + n_samples) of ring float32 [N_RX, ant_stride, 2], then noise and the ADC
        (AdcCfg or None). ring_len: samples per ring turn when the rows are longer (default: the row)."""
        import torch
        dev = int(self.cfg.device)
        n_em = len(emissions)
        self._check_ring(ring, 1)
        ring_len = ring.shape[1] if ring_len is None else int(ring_len)
        if not 0 < ring_len <= ring.shape[1]:
            raise ValueError(f"ring_len {ring_len} outside the ring rows ({ring.shape[1]} samples)")
        if tx is None:
            if n_em:
                raise ValueError("vspace_mix: emissions without tx samples")
            n_tx, n_rows, S_tx, tx_p = 1, 0, 0, None
        else:
            _check_tensor(tx, "tx", torch.float32, 4, dev)
            if tx.shape[3] != 2:
                raise ValueError(f"tx shape {tuple(tx.shape)}, expected [n_rows, N_TX, S_tx, 2]")
            n_rows, n_tx, S_tx, tx_p = tx.shape[0], tx.shape[1], tx.shape[2], C.c_void_p(tx.data_ptr())
        arr = emissions if isinstance(emissions, C.Array) else (VspaceEmission * n_em)(*emissions)
        _chk(lib().dnrp_vspace_mix(self._ctx, C.byref(cfg), C.byref(adc) if adc is not None else None, n_em,
                                   C.cast(arr, C.c_void_p) if n_em else None, n_tx, tx_p, n_rows, S_tx, ring.shape[0],
                                   C.c_void_p(ring.data_ptr()), ring_len, ring.shape[1], int(t_begin), int(n_samples),
                                   _stream_ptr(stream)), "dnrp_vspace_mix")

    def chscan(self, ring, reqs, n_ant=None, stream=None, ring_len=None):
        """Channel scanner (dnrp_chscan_batch, chscanner_t::scan) over ring float32 [N_ant, ant_stride, 2]:
        returns (list of float32 arrays of the requests' partial RMS values, rms_avg float32 [n] = the
        sum of each request's partial values, as chscan_t::rms_avg)."""
        n_ant = n_ant or ring.shape[0]
        self._check_ring(ring, n_ant)
        ring_len = ring.shape[1] if ring_len is None else int(ring_len)
        if not 0 < ring_len <= ring.shape[1]:
            raise ValueError(f"ring_len {ring_len} outside the ring rows ({ring.shape[1]} samples)")
        n = len(reqs)
        arr = reqs if isinstance(reqs, C.Array) else (ChscanReq * n)(*reqs)
        counts = np.array([arr[i].N_partial for i in range(n)], np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(counts, out=off[1:])
        if off[-1] > 0x7FFFFFFF:
            raise ValueError("chscan: too many partial scans")
        off32 = np.ascontiguousarray(off[:-1].astype(np.uint32))
        part = np.zeros(max(1, int(off[-1])), np.float32)
        avg = np.zeros(max(1, n), np.float32)
        _chk(lib().dnrp_chscan_batch(self._ctx, C.c_void_p(ring.data_ptr()), ring_len, ring.shape[1], n_ant, n,
                                     C.cast(arr, C.c_void_p) if n else None, C.c_void_p(part.ctypes.data),
                                     C.c_void_p(off32.ctypes.data), C.c_void_p(avg.ctypes.data), _stream_ptr(stream)),
             "dnrp_chscan_batch")
        return [part[int(off[i]):int(off[i + 1])] for i in range(n)], avg[:n]

    def sync_stream_init(self, sc):
        state = SyncStreamState()
        _chk(lib().dnrp_sync_stream_init(self._ctx, C.byref(sc), C.byref(state)), "dnrp_sync_stream_init")
        return state

    def sync_stream_window(self, sc):
        return int(lib().dnrp_sync_stream_window(self._ctx, C.byref(sc)))

    def rx_sync_stream(self, sc, ring, t0, n_chunks, state, stream=None):
        """Continuous-stream sync of n_chunks chunks from global time t0 over the ring; returns the
        unique reports (SYNC_RESULT_DTYPE, global times) and the chunk each was found in."""
        self._check_ring(ring, sc.N_ant_limited)
        out = np.zeros(max(1, n_chunks * sc.max_reports), SYNC_RESULT_DTYPE)
        chunk_of = np.zeros(max(1, n_chunks * sc.max_reports), np.uint32)
        n_out = C.c_uint32()
        _chk(lib().dnrp_rx_sync_stream(self._ctx, C.byref(sc), C.c_void_p(ring.data_ptr()), ring.shape[1],
                                       ring.shape[1], int(t0), n_chunks, C.byref(state), C.c_void_p(out.ctypes.data),
                                       C.byref(n_out), C.c_void_p(chunk_of.ctypes.data), _stream_ptr(stream)),
             "dnrp_rx_sync_stream")
        return out[: n_out.value], chunk_of[: n_out.value]

    def kernel_time_total(self, name, reset=True):
        ms, cnt = C.c_float(), C.c_uint32()
        _chk(lib().dnrp_kernel_time_total(self._ctx, name.encode(), C.byref(ms), C.byref(cnt), int(reset)),
             "dnrp_kernel_time_total")
        return float(ms.value), int(cnt.value)

    def last_kernel_ms(self, name):
        ms = C.c_float()
        _chk(lib().dnrp_last_kernel_ms(self._ctx, name.encode(), C.byref(ms)), "dnrp_last_kernel_ms")
        return float(ms.value)
