/*
 * dnrp.h — C-ABI of the MI355X-native DECT NR+ lower PHY (libdnrp.so).
 *
 * Drop-in boundary for the OFDM TX/RX hot path of maxpenner/DECT-NR-Plus-SDR. The reference has
 * no FFI; its path is three C++ classes owned per worker thread. Each entry point below replaces
 * one of them, batched over many independent packets (slots):
 *
 *   dnrp_ctx_create        <- tx_rx_t / tx_t / rx_synced_t constructors
 *                             (lib/src/phy/tx_rx.cpp:38-129, tx/tx.cpp:48-141,
 *                              rx/rx_synced/rx_synced.cpp:55-174)
 *   dnrp_add_network_id    <- tx_rx_t::add_new_network_id (lib/include/dectnrp/phy/tx_rx.hpp:52,
 *                             sections_part3/scrambling_pdc.cpp:36-57)
 *   dnrp_get_packet_sizes  <- sp3::get_packet_sizes (sections_part3/derivative/packet_sizes.cpp:99)
 *   dnrp_compute_packet_sizes  (same, context-free and host-only)
 *   dnrp_tx_batch          <- tx_t::generate_tx_packet (lib/include/dectnrp/phy/tx/tx.hpp:80-81,
 *                             lib/src/phy/tx/tx.cpp:165-314), FEC boundary between rate matching
 *                             and scrambling (pcc_enc.cpp:212, pdc_enc.cpp:218-221)
 *   dnrp_rx_sync_batch     <- sync_chunk_t::search() per window (lib/include/dectnrp/phy/rx/sync/
 *                             sync_chunk.hpp:72, lib/src/phy/rx/sync/sync_chunk.cpp:143-279)
 *   dnrp_rx_pcc_batch      <- rx_synced_t::demoddecod_rx_pcc up to the descrambled PCC d-bits
 *                             (lib/include/dectnrp/phy/rx/rx_synced/rx_synced.hpp:93,
 *                              rx_synced.cpp:186-302, pcc_enc.cpp:297)
 *   dnrp_rx_pdc_batch      <- rx_synced_t::demoddecod_rx_pdc up to the descrambled PDC d-bits
 *                             (rx_synced.hpp:103, rx_synced.cpp:325-436, pdc_enc.cpp:339-344)
 *   dnrp_ctx_destroy       <- destructors
 *
 * Conventions (all functions):
 *   - return 0 on success, a negative DNRP_E* code on argument/configuration error; never abort.
 *   - bulk buffers (bits, IQ, LLRs) are DEVICE pointers on the context's HIP device; descriptor
 *     and report arrays are HOST pointers. IQ is interleaved cf32, one contiguous stream per
 *     antenna (radio/complex.hpp:28, buffer_tx.hpp, buffer_rx.hpp).
 *   - work is stream-ordered on the caller's hipStream_t (passed as void*, NULL = default
 *     stream); host report arrays are valid after dnrp_sync() or a stream synchronisation.
 *   - one context per submitting host thread; contexts are not thread-safe (like the reference's
 *     per-worker tx_t/rx_synced_t objects).
 *   - LLRs are int16, positive means bit 1 (phy_config.hpp:39-41, fec/test/tb2pdc.cpp:173-176).
 */
#ifndef DNRP_H
#define DNRP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNRP_OK 0
#define DNRP_EINVAL (-1)      /* bad argument / null pointer */
#define DNRP_ECONFIG (-2)     /* packet configuration not valid (get_packet_sizes -> nullopt) */
#define DNRP_EUNSUPPORTED (-3)/* valid DECT NR+ configuration the reference RX cannot demodulate */
#define DNRP_ENOMEM (-4)      /* device allocation failed / batch larger than max_batch */
#define DNRP_EDEVICE (-5)     /* HIP runtime error */
#define DNRP_ENETID (-6)      /* network ID not registered with dnrp_add_network_id */
#define DNRP_ESTATE (-7)      /* dnrp_rx_pdc_batch without a preceding dnrp_rx_pcc_batch; dnrp_rx_sync_fine_peaks
                                 or dnrp_rx_sync_icfo_scores without a preceding dnrp_rx_sync_batch that ran with
                                 the setting on;
                                 dnrp_rx_mimo_detail without a preceding dnrp_rx_pdc_batch that ran with detail = 1;
                                 dnrp_rx_aoa without a preceding dnrp_rx_pdc_batch that ran with the report on */

typedef struct dnrp_ctx dnrp_ctx;

/* worker_pool_config_t subset (phy/worker_pool_config.hpp) */
typedef struct {
    uint32_t u_max, b_max;      /* radio device class maxima (sections_part3/radio_device_class.cpp) */
    uint32_t N_TX_max;          /* physical antennas; RX uses N_RX = N_TX_max (rx_synced.hpp:120-126) */
    uint32_t os_min;            /* minimum oversampling (phy.json os_min) */
    uint32_t L, M;              /* hw/DECT resampling ratio L/M for TX, M/L for RX (phy_config.cpp:28-94) */
    uint32_t chestim_mode_lr;   /* phy.json chestim_mode_lr_default */
    uint32_t chestim_lr_stride; /* phy.json chestim_mode_lr_t_stride_default */
    uint32_t max_batch;         /* packets per batch call */
    int32_t device;             /* HIP device ordinal */
} dnrp_cfg;

/* sp3::packet_sizes_def_t */
typedef struct {
    uint32_t u, b, PacketLengthType, PacketLength, tm_mode_index, mcs_index, Z;
} dnrp_psdef;

/* sp3::packet_sizes_t + context-dependent hw-rate sizes */
typedef struct {
    uint32_t N_PACKET_symb, N_DF_symb, N_PDC_subc, N_DRS_subc, G, N_PDC_bits, N_TB_bits, N_TB_byte, C;
    uint32_t N_samples_STF, N_samples_STF_CP_only, N_samples_DF, N_samples_GI;
    uint32_t N_samples_packet_no_GI, N_samples_packet;
    uint32_t N_bps, N_eff_TX, N_SS, N_TS, N_TX, N_b_DFT, N_b_OCC;
    uint32_t N_b_DFT_os;                  /* FFT size used (tx.cpp:439) */
    uint32_t N_samples_packet_no_GI_os_rs;/* hw samples carrying the packet (tx.cpp:527-529) */
    uint32_t N_samples_packet_os_rs;      /* hw samples of the slot window incl. full GI */
} dnrp_packet_sizes;

/* tx_descriptor_t + tx_meta_t subset (phy/tx/tx_descriptor.hpp, phy/tx/tx_meta.hpp) */
typedef struct {
    uint32_t codebook_index;
    uint32_t network_id;      /* must have been registered */
    uint32_t plcf_type;       /* 1 or 2: selects the PDC scrambling sequence */
    uint32_t GI_percentage;   /* share of the GI actually transmitted (zeros) */
    float DAC_scale;
    float iq_phase_rad;
    float iq_phase_increment_s2s_post_resampling_rad;
    uint32_t optimal_scaling_DAC; /* 0: standard W scaling, 1: W_t::scaling_factor_optimal_DAC (tx.cpp:582-592) */
} dnrp_tx_desc;

/* sync_report_t fields consumed by rx_synced_t (phy/rx/sync/sync_report.hpp) */
typedef struct {
    int64_t fine_peak_time;   /* hw-rate sample index of the packet start inside its window */
    float cfo_fractional_rad; /* per DECT-rate sample */
    float cfo_integer_rad;    /* per DECT-rate sample, added to cfo_fractional_rad: 0, or -k 8 pi / N_b_DFT_os of
                                 dnrp_ctx_set_sync_icfo_search */
    uint32_t u, b, N_eff_TX;
    uint32_t window;          /* window of iq_in holding the packet (the sync window it was found in:
                                 several packets of one window share it) */
    float rms[8];             /* sync_report_t::rms_array (dnrp_sync_result::rms_array): the RX keeps
                                 the values > 0 and estimates the others over the STF
                                 (RX_SYNCED_PARAM_RMS_KEEP_VALUES_PROVIDED_BY_SYNC, rx_synced.cpp:620-655) */
} dnrp_sync_report;

/* Synchronisation of one batch of windows (sync_chunk_t, worker_pool_config_t subset) */
typedef struct {
    uint32_t u, b;          /* radio device class u_min / b_min: the STF searched for (sync_chunk.cpp:54-57) */
    uint32_t N_ant_limited; /* antennas searched, <= cfg.N_TX_max (RX_SYNC_PARAM_AUTOCORRELATOR_ANTENNA_LIMIT) */
    uint32_t chunk_len;     /* hw samples per chunk; the search covers chunk_len/L*M + 4 STFs at the
                               DECT rate (sync_chunk.cpp:63-66), the window must hold the peak and
                               cross-correlation samples after it (zeros are read past S_win) */
    uint32_t max_reports;   /* packets reported per window (successive search() calls on one chunk) */
} dnrp_sync_cfg;

/* sync_report_t (phy/rx/sync/sync_report.hpp:29-98) of one synchronised packet. "local" times are
 * DECT-rate sample indices of the chunk's resampled buffer, the others hw sample indices relative
 * to the window start. fine_peak_time / cfo_fractional_rad / cfo_integer_rad / u / b / N_eff_TX are
 * what dnrp_rx_pcc_batch consumes (as a dnrp_sync_report). */
typedef struct {
    uint32_t found;                   /* 1: packet synchronised; 0: slot unused */
    uint32_t detection_ant_idx;
    float detection_rms, detection_metric;
    uint32_t detection_time_local, detection_time_with_jump_back_local;
    uint32_t coarse_peak_time_local, fine_peak_time_local;
    int64_t coarse_peak_time;
    int64_t fine_peak_time;
    float coarse_peak_array[8];       /* > 0: antenna had a valid coarse peak (its smoothed metric) */
    float rms_array[8];
    float cfo_fractional_rad, cfo_integer_rad;
    uint32_t u, b, N_eff_TX, reserved;
    float fine_peak_metric[4];        /* |xcorr| maximum per STF template N_eff_TX = 1, 2, 4, 8 */
    uint32_t fine_peak_index[4];
} dnrp_sync_result;

/* PHY part of pcc_report_t plus the sync_report_t values rx_synced_t refines (rx_synced.cpp:530-580) */
typedef struct {
    float snr_dB;             /* estimator_snr after STF + DRS of the PCC symbols */
    float cfo_fractional_rad; /* sync value + STF re-estimate */
    float sto_fractional;     /* samples, estimator_sto on the STF */
    float rms[8];             /* per RX antenna: the sync report's value where > 0, else the STF estimate */
} dnrp_pcc_report;

/* PHY part of pdc_report_t (rx_synced.cpp:432-435) with its mimo_report_t
 * (phy/rx/rx_synced/mimo/mimo_report.hpp; estimator_mimo.cpp:80-222) */
typedef struct {
    float snr_dB;
    uint32_t mimo_N_RX;                          /* own physical antennas */
    uint32_t mimo_N_TS_other;                    /* transmit streams received (N_eff_TX) */
    uint32_t tm_3_7_beamforming_idx;             /* codebook index recommended to the other side */
    uint32_t tm_3_7_beamforming_reciprocal_idx;  /* codebook index for this side if reciprocal */
} dnrp_pdc_report;

/* Per-packet PDC request = what maclow_phy_t carries once the MAC has decided from the decoded PLCF
 * to continue with the PDC (phy/interfaces/maclow_phy.hpp: continue_with_pdc, hp_rx): the HARQ
 * process' packet configuration (harq::process_rx_t::get_packet_sizes -> psdef), network ID and
 * PLCF type (rx_synced.cpp:325-350), plus the packet's slot in the preceding dnrp_rx_pcc_batch
 * (the rx_synced_t state the reference keeps between demoddecod_rx_pcc and demoddecod_rx_pdc).
 * Packets the MAC rejected (continue_with_pdc = false) are simply not requested. */
typedef struct {
    dnrp_psdef psdef;     /* u, b and N_eff_TX (tm_mode_index) must match the PCC slot's sync report */
    uint32_t pcc_index;   /* slot index i of sr[i] in the preceding dnrp_rx_pcc_batch, each at most once */
    uint32_t network_id;
    uint32_t plcf_type;   /* 1 or 2: selects the PDC descrambling sequence (scrambling_pdc.cpp:41-48) */
} dnrp_pdc_req;

int dnrp_ctx_create(const dnrp_cfg* cfg, dnrp_ctx** out);
int dnrp_ctx_destroy(dnrp_ctx* ctx);
int dnrp_add_network_id(dnrp_ctx* ctx, uint32_t network_id);
int dnrp_get_packet_sizes(const dnrp_ctx* ctx, const dnrp_psdef* psdef, dnrp_packet_sizes* out);
/* Same as dnrp_get_packet_sizes without a context or device: the reference's static
 * sp3::get_packet_sizes (sections_part3/derivative/packet_sizes.cpp:99-236). The oversampled /
 * resampled fields (N_b_DFT_os, N_samples_packet_*_os_rs) are filled from cfg when cfg is not
 * NULL (tx.cpp:429-600 geometry), else 0. Host-only: safe on machines without a GPU. */
int dnrp_compute_packet_sizes(const dnrp_cfg* cfg, const dnrp_psdef* psdef, dnrp_packet_sizes* out);

/*
 * TX: n packets of one configuration.
 *   pcc_d   device [n][25] bytes: 196 rate-matched PCC bits, unscrambled, MSB first
 *   pdc_d   device [n][pdc_stride] bytes: G rate-matched PDC bits, unscrambled, MSB first
 *   iq_out  device [n][N_TX][S] cf32; samples [0, N_samples_packet_no_GI_os_rs) carry the packet,
 *           the rest (GI and slot tail) are written as zeros. S >= N_samples_packet_os_rs.
 */
int dnrp_tx_batch(dnrp_ctx* ctx, const dnrp_psdef* psdef, uint32_t n, const dnrp_tx_desc* desc,
                  const uint8_t* pcc_d, const uint8_t* pdc_d, uint32_t pdc_stride, float* iq_out,
                  uint32_t S, void* stream);

/*
 * TX OFDM windowing <- the build option PHY_TX_OFDM_WINDOWING (lib/include/dectnrp/phy/tx/tx.hpp:38,
 * lib/src/phy/tx/tx.cpp:66-79,126-132,881-908, lib/src/phy/dft/windowing.cpp:34-56): per antenna
 * stream at the DECT rate, ahead of the resampler, the first N samples of every data-field symbol's
 * cyclic prefix are multiplied by a rising raised-cosine edge and the cyclic continuation of the
 * symbol before it (the first N samples of that symbol's body, the STF's taken ahead of its cover
 * sequence as in tx.cpp:226-234) is added, multiplied by the mirrored edge. The STF's own prefix and
 * the sample counts do not change. N = roundf(N_b_DFT_os / 8 * fraction) for the STF too.
 *   fraction  0 (default): off, exactly the transmitter without the option; (0, 1]: on for every later
 *             dnrp_tx_batch of the context (no context rebuild). DNRP_EINVAL for a NULL context, a
 *             negative, > 1 or non-finite value.
 * With windowing on, dnrp_tx_batch returns DNRP_EINVAL for a packet whose N would be below 2 (the
 * reference asserts it, windowing.cpp:39), before any work is queued.
 */
int dnrp_ctx_set_tx_windowing(dnrp_ctx* ctx, float fraction);

/*
 * Host only: the rising edge rc[n] = cos((n - N) / N * pi / 2)^2, n = 0..N-1, in float
 * (lib/src/phy/filter/raised_cosine.cpp:30-56) of an N_b_DFT_os-point symbol at `fraction` -- the
 * table the device uses; the falling edge is rc[N - 1 - n]. Returns N; rising may be NULL to ask for
 * the length. DNRP_EINVAL for N_b_DFT_os % 8 != 0, a fraction outside (0, 1], N < 2 or cap < N.
 */
int dnrp_tx_window(uint32_t N_b_DFT_os, float fraction, float* rising, uint32_t cap);

/*
 * The kernel form a dnrp_tx_batch launches, chosen from the packet geometry, the output buffer and the
 * context's settings by one host function. dnrp_tx_batch has one timer ("tx"); this read-back is how a test
 * proves which instantiation it ran.
 *   family     DNRP_TX_FORM_STREAM: the streaming kernel (N_b_DFT_os = 1024 at 10/9, os_min 1, 9 STF patterns,
 *              even S, iq_out 16-byte aligned, every symbol's PDC bytes inside its staging window);
 *              DNRP_TX_FORM_WAVE: one wavefront per symbol, N_b_DFT_os = 1024 otherwise;
 *              DNRP_TX_FORM_BLOCK: one workgroup per symbol run, N_b_DFT_os < 1024;
 *              DNRP_TX_FORM_SCRATCH: symbols through a DECT-rate scratch, N_b_DFT_os > 1024
 *   L, M, hl   resampler ratio and half length compiled into the instantiation: 10/9/22 (os_min 1), 10/9/4
 *              (os_min 2), 1/1/0; 0/0/0: the form that takes them at run time (40/27, and the scratch family)
 *   windowed   1 with dnrp_ctx_set_tx_windowing on
 *   stream:    mode 0 SISO (N_TS = 1), 1 transmit diversity, 2 spatial multiplexing, 3 / 4 the same two where
 *              every antenna row of every packet's W has one nonzero entry; q8: 256-QAM form; mfma: DNRP_TX_MFMA;
 *              sb_chunks: KiB of a symbol's PDC byte window; n_seg: segments per antenna stream
 *   wave, block: staged 1 where a symbol run's PDC bytes (<= 8192) are staged in LDS, 0 where they are read in place
 *   scratch:   passes of the batch through the scratch (DNRP_TX_BIG_CAP)
 * Fields of the other families are 0.
 * dnrp_tx_last_form: the form of the context's latest dnrp_tx_batch that launched; DNRP_ESTATE before the first.
 * dnrp_tx_form_for: host only, no context or device: the form dnrp_tx_batch would take for n packets of psdef
 * with the codebook indices codebook[n], row length S, iq_out at an address congruent to out_misalign modulo
 * 16, windowing fraction win_fraction (0: off), under the same environment switches. The errors are
 * dnrp_tx_batch's for the same arguments.
 */
#define DNRP_TX_FORM_STREAM 0u
#define DNRP_TX_FORM_WAVE 1u
#define DNRP_TX_FORM_BLOCK 2u
#define DNRP_TX_FORM_SCRATCH 3u
typedef struct {
    uint32_t family, L, M, hl, windowed;
    uint32_t mode, q8, mfma, sb_chunks, n_seg;
    uint32_t staged;
    uint32_t passes;
} dnrp_tx_form;
int dnrp_tx_last_form(const dnrp_ctx* ctx, dnrp_tx_form* out);
int dnrp_tx_form_for(const dnrp_cfg* cfg, const dnrp_psdef* psdef, uint32_t n, const uint32_t* codebook, uint32_t S,
                     uint32_t out_misalign, float win_fraction, dnrp_tx_form* out);

/*
 * Synchronisation: sync_chunk_t::search() on n windows, each window one chunk whose sync resampler
 * starts with zero history at sample 0 (reset_localbuffer, sync_chunk.cpp:300-311). Detection,
 * coarse peak and fine peak as in the reference; up to max_reports packets per window in search
 * order (the reference returns them from successive search() calls).
 *   iq       device cf32; window w, antenna a, sample i at iq[2*(w*win_stride + a*ant_stride + i)]
 *            (strides in samples: [n][N_RX][S] windows or per-antenna continuous streams)
 *   res      host [n][max_reports]; n_found host [n] (optional). Valid after dnrp_sync().
 * DNRP_EUNSUPPORTED for a sync geometry (sc->u, sc->b with the context's os_min, L and M) whose detection
 * staging or whose fine search (two buffers of the power of two >= xc_len - 1 + tmpl_len points) exceeds
 * 160 KiB of LDS, e.g. (u 2, b 16) at os_min 2 and 40/27: nothing is queued, the context stays usable.
 */
int dnrp_rx_sync_batch(dnrp_ctx* ctx, const dnrp_sync_cfg* sc, uint32_t n, const float* iq, uint64_t win_stride,
                       uint64_t ant_stride, uint32_t S_win, dnrp_sync_result* res, uint32_t* n_found, void* stream);

/*
 * Beta search at the coarse peak <- the build option
 * RX_SYNC_PARAM_AUTOCORRELATOR_PEAK_FIND_BETA_THRESHOLD_DB_OR_ASSUME_MAX_OF_RDC
 * (lib/include/dectnrp/phy/rx/sync/sync_param.hpp:238-244, off by default there too). A receiver of a class
 * with b_max is triggered by packets of every b <= b_max; with the search on, the synchronisation finds
 * the packet's b and cross-correlates against the STF templates of that b:
 *  - coarse_peak_f_domain_t::process / estimate_beta (lib/src/phy/rx/sync/coarse_peak_f_domain.cpp:70-193):
 *    for every searched antenna the N = 64 b_max os_min DECT-rate samples starting
 *    N_samples_STF_CP_only_os after coarse_peak_time_local are transformed (no CFO correction), and after
 *    the FFT shift, from b = 1 (bins [N/2 - 32, N/2 + 32)), the next b' of b_idx2b = {1, 2, 4, 8, 12, 16}
 *    is taken while (side / (2 n_side)) / (centre / (64 b)) > threshold_linear, the sideband being the
 *    n_side = (b' - b) 32 bins on either side of the current band, powers summed over the antennas;
 *  - stf_template_t (lib/src/phy/rx/sync/stf_template.cpp:137-199): templates of every b <= b_max at the
 *    class rate; the fine search takes the rows of the report's b (crosscorrelator.cpp:159).
 * dnrp_sync_cfg::b stays the class maximum whose sample rate the stream has; the candidates are the
 * values of b_idx2b <= it, and the search ends there (the reference's loop would test one b further and
 * stops in its asserts). cfo_integer_rad is the business of dnrp_ctx_set_sync_icfo_search below: the decision
 * here reads the uncorrected band powers and comes first, the integer CFO search uses the decided b, and a
 * report whose integer CFO is k != 0 has its b decided again from the spectrum moved back by 4 k bins. With both
 * searches on, the b of such a report is therefore not the reference's estimate_beta on the raw spectrum but that
 * estimator on the spectrum with the integer CFO taken out (this project's divergence); for k = 0, and with the
 * integer CFO search off, it is the reference's.
 *   on            0 (default): exactly the synchronisation without the option, b = dnrp_sync_cfg::b, the
 *                 same templates, no further launch. 1: on for every later dnrp_rx_sync_batch and
 *                 dnrp_rx_sync_stream of the context (no context rebuild); the templates of the other b
 *                 are built at the first such call per (u, b).
 *   threshold_db  the reference's value is -10. threshold_linear = 10^(dB / 20): the reference converts
 *                 with db2mag and compares a power ratio against it (coarse_peak_f_domain.cpp:143-144,177);
 *                 mirrored, not repaired.
 * DNRP_EINVAL for a NULL context, on > 1 or a non-finite threshold_db. The getter's outputs may be NULL.
 */
int dnrp_ctx_set_sync_beta_search(dnrp_ctx* ctx, uint32_t on, float threshold_db);
int dnrp_ctx_get_sync_beta_search(const dnrp_ctx* ctx, uint32_t* on, float* threshold_db, float* threshold_linear);

/*
 * Fine search over every antenna that has a coarse peak <- the build option
 * RX_SYNC_PARAM_CROSSCORRELATOR_ALL_ANTENNAS_OR_ONLY_STRONGEST
 * (lib/include/dectnrp/phy/rx/sync/sync_param.hpp:286; crosscorrelator_t::run_fine_search,
 * lib/src/phy/rx/sync/crosscorrelator.cpp:122-249).
 *   on  0 (default): exactly the synchronisation without the option: the antenna with the largest
 *       coarse_peak_array entry is cross-correlated against the STF templates, the same launch, byte-identical
 *       reports.
 *       1: for every later dnrp_rx_sync_batch and dnrp_rx_sync_stream of the context (no context rebuild) every
 *       searched antenna whose coarse_peak_array entry is > 0 is cross-correlated against every template
 *       (crosscorrelator.cpp:137-147, 165-203), and of a report
 *         fine_peak_metric[k]   is the reference's metric_sum of template k: the float sum of the processed
 *                               antennas' metrics in ascending antenna order (crosscorrelator.cpp:221-226);
 *         fine_peak_index[k]    roundf(sum_a metric[a][k] index[a][k] / metric_sum[k]), relative to the search
 *                               start coarse_peak_time - search_left as before, rounded once;
 *         N_eff_TX              1 << argmax_k metric_sum[k], strictly greater from 0, so the first template of a
 *                               tie (crosscorrelator.cpp:218-233);
 *         fine_peak_time_local  fine_peak_index[k_likely] (crosscorrelator.cpp:239-248), and fine_peak_time =
 *                               coarse_peak_time - search_left + fine_peak_time_local.
 *       Every other field, and the number and order of the reports, is as with the setting off (the search
 *       goes on from the coarse peak). With one searched antenna the reports equal the off path's bit for bit.
 *       Independent of dnrp_ctx_set_sync_beta_search: with both on every antenna is correlated against the
 *       template rows of the decided b.
 * DNRP_EINVAL for a NULL context or on > 1. The getter's output may be NULL.
 *
 * dnrp_rx_sync_fine_peaks: stream-ordered copy of the per-antenna peaks (peak_vec, crosscorrelator.cpp:195-201)
 * of the context's latest dnrp_rx_sync_batch, which must have run with the setting on. metric and index are
 * host arrays [n_reports][8][4] ordered (report slot in `res` order, antenna, template); n_reports must equal
 * that call's n * max_reports. index is relative to the search start. Entries of antennas that were not
 * processed are 0: antennas without a coarse peak, antennas >= N_ant_limited, templates the class does not
 * have, slots not `found`. Valid once `stream` has been synchronised. Not offered for dnrp_rx_sync_stream,
 * which filters and reorders the reports of its chunks: after it the call returns DNRP_ESTATE.
 * DNRP_ESTATE if the latest sync call ran with the setting off or there was none; DNRP_EINVAL for a NULL
 * pointer or another n_reports.
 */
int dnrp_ctx_set_sync_fine_all_antennas(dnrp_ctx* ctx, uint32_t on);
int dnrp_ctx_get_sync_fine_all_antennas(const dnrp_ctx* ctx, uint32_t* on);
int dnrp_rx_sync_fine_peaks(dnrp_ctx* ctx, uint32_t n_reports, float* metric, uint32_t* index, void* stream);

/*
 * Integer CFO search at the coarse peak <- the build option
 * RX_SYNC_PARAM_AUTOCORRELATOR_PEAK_FIND_INTEGER_CFO_SEARCH_RANGE_OR_ASSUME_ZERO
 * (lib/include/dectnrp/phy/rx/sync/sync_param.hpp:245-252), whose estimator the reference leaves as
 * `#error "integer CFO not implemented yet"` (lib/src/phy/rx/sync/coarse_peak_f_domain.cpp:195-199). The
 * estimator is this project's own. cfo_fractional_rad is unambiguous within +-2 subcarriers
 * only (the STF patterns are N/4 samples apart); an offset of (4 k + f) subcarriers leaves f there and k
 * unseen, and the fine search then misses the peak and N_eff_TX. With the search on, for every searched
 * antenna the N = 64 b os_min DECT-rate samples the beta search transforms (the STF's last N at the coarse
 * peak) are multiplied by their patterns' cover-sequence signs and by exp(j cfo_fractional_rad i), transformed,
 * and candidate k scores the power on the bins 4 (i + k) mod N, 0 < |i| <= N_b_OCC(b') / 8, b' the report's b
 * (the decided b with the beta search on). A candidate with 4 (N_b_OCC(b') / 8 + |k|) >= N / 2 is not
 * searched. The scores are summed over the antennas in antenna order in float; the candidates are visited
 * 0, -1, +1, -2, ... and a later one wins only if strictly greater. Then
 *   cfo_integer_rad = (float)(-k 4 2 pi / N)   (+0 for k = 0),
 * a correction with the sign of cfo_fractional_rad, the fine search pre-corrects with the sum of both, and
 * dnrp_rx_pcc_batch mixes with the sum as before.
 *   range  0 (default): exactly the synchronisation without the option: no further launch, cfo_integer_rad = 0,
 *          byte-identical reports. 1..4: k in [-range, range] for every later dnrp_rx_sync_batch and
 *          dnrp_rx_sync_stream of the context (no context rebuild).
 * DNRP_EINVAL for a NULL context or range > 4. The getter's output may be NULL.
 *
 * dnrp_rx_sync_icfo_scores: the score table and the decided k of the context's latest dnrp_rx_sync_batch, which
 * must have run with the search on. score is a host array [n_reports][8][9] ordered (report slot in `res`
 * order, antenna, candidate k + 4), k a host array [n_reports]; n_reports must equal that call's
 * n * max_reports. -1 in the columns outside the range or not searched, in the rows of antennas >=
 * N_ant_limited and of slots not `found` (their k is 0). Synchronises `stream` before it returns. Not offered
 * for dnrp_rx_sync_stream (DNRP_ESTATE after it). DNRP_ESTATE if the latest sync call ran with the search off
 * or there was none; DNRP_EINVAL for a NULL pointer or another n_reports.
 */
int dnrp_ctx_set_sync_icfo_search(dnrp_ctx* ctx, uint32_t range);
int dnrp_ctx_get_sync_icfo_search(const dnrp_ctx* ctx, uint32_t* range);
int dnrp_rx_sync_icfo_scores(dnrp_ctx* ctx, uint32_t n_reports, float* score, int32_t* k, void* stream);

/*
 * RX phase 1: synchronised PCC demodulation of n packets. Each packet is processed with the
 * (u, b, N_eff_TX) of its own sync report (packets are grouped internally, like independent
 * demoddecod_rx_pcc calls).
 *   sr       host [n]; packet i lies in window sr[i].window of iq_in at sr[i].fine_peak_time (may
 *            be negative: zero history before the window start)
 *   iq_in    device [n_windows][N_RX][S_in] cf32, N_RX = cfg.N_TX_max; DNRP_EINVAL if any
 *            sr[i].window >= n_windows (the kernels read window sr[i].window of iq_in)
 *   pcc_llr  device [n][196] int16, descrambled
 *   rep      host [n] (optional)
 * Device state for phase 2 (STF estimates, PCC-phase channel estimates) is kept in the context
 * until the next dnrp_rx_pcc_batch.
 */
int dnrp_rx_pcc_batch(dnrp_ctx* ctx, uint32_t n, const dnrp_sync_report* sr, const float* iq_in,
                      uint32_t n_windows, uint32_t S_in, int16_t* pcc_llr, dnrp_pcc_report* rep, void* stream);

/*
 * RX phase 2: PDC demodulation of any subset of the packets of the preceding dnrp_rx_pcc_batch,
 * each with its own PLCF-announced configuration (mixed MCS / PacketLength / network IDs are
 * grouped internally).
 *   req      host [m], m <= n of the PCC batch, distinct pcc_index values
 *   iq_in    the PCC call's iq_in, n_windows and S_in: the PDC symbols are read from these windows,
 *            so they must stay valid and unchanged until this call's work has completed
 *   pdc_llr  device [m][llr_stride] int16: row r = the G descrambled LLRs of req[r]
 *   rep      host [m] (optional)
 * Returns DNRP_ESTATE without a preceding PCC batch or for an iq_in / n_windows other than the
 * PCC call's, DNRP_EINVAL for a pcc_index out of range or repeated, a psdef whose u/b/N_eff_TX
 * differ from the slot's sync report, S_in different from the PCC call, or llr_stride < G.
 */
int dnrp_rx_pdc_batch(dnrp_ctx* ctx, uint32_t m, const dnrp_pdc_req* req, const float* iq_in, uint32_t n_windows,
                      uint32_t S_in, int16_t* pdc_llr, uint32_t llr_stride, dnrp_pdc_report* rep, void* stream);

int dnrp_sync(dnrp_ctx* ctx, void* stream);

/*
 * Receiver options beyond the reference (default 0: exactly the reference's receiver).
 *   DNRP_RX_MODE_SM_MMSE  dnrp_rx_pdc_batch demodulates spatial multiplexing (N_SS = N_eff_TX in
 *                         {2, 4}: TM 2/4/6/8/9, N_RX >= N_SS) by linear MMSE per cell, x = (H^H H +
 *                         nv I)^-1 H^H y with the Wiener-interpolated channel of every transmit stream
 *                         and the SNR estimator's noise variance nv, unbiased per stream, then the same
 *                         soft demapper. The reference leaves run_pdc_mode_AxA_MIMO empty
 *                         (rx_synced.cpp:1331-1333) and returns DNRP_EUNSUPPORTED without this flag.
 * Takes effect for the next dnrp_rx_pcc_batch (a preceding PCC batch's state is dropped).
 */
#define DNRP_RX_MODE_SM_MMSE 1u
int dnrp_ctx_set_rx_mode(dnrp_ctx* ctx, uint32_t flags);

/*
 * Residual STO tracking from the DRS symbols <- the build option RX_SYNCED_PARAM_STO_RESIDUAL_BASED_ON_DRS
 * (lib/include/dectnrp/phy/rx/rx_synced/rx_synced_param.hpp:156; rx_synced.cpp:767-770, 839-841,
 * estimator_sto.cpp:64-97, 148-171), which the reference's default build leaves out.
 *   on  0 (default): exactly the receiver without the option: every symbol of a packet is derotated with
 *       the STO increment estimated from the STF, the same launches, byte-identical LLRs and reports.
 *       1: after every DRS symbol the slope over frequency of its zero-forced pilots -- per RX antenna and
 *       transmit stream TS_first..min(TS_last, 7) the angle of sum_i h[i] conj(h[i + 1]) over the stream's
 *       DRS cells divided by 4, averaged over (antenna, stream) -- times `gain` is added to the running
 *       increment, and every later symbol is derotated with the new value (a DRS symbol itself with the
 *       value from before its own update). This follows a sampling-clock offset over a long packet. The
 *       PDC phase continues from the PCC phase's state. The fused receiver (DNRP_RX_FUSED) and the grouped
 *       Y path (DNRP_RX_GROUP) are not taken while it is on.
 *   gain  scales each residual before it is added: 1 is the reference, 0 runs the whole mechanism with
 *       every symbol's increment equal to the STF estimate (LLRs byte-identical to off).
 * Read once per dnrp_rx_pcc_batch; that call's dnrp_rx_pdc_batch takes the same values. With it on, a
 * dnrp_rx_pdc_batch request for spatial multiplexing (DNRP_RX_MODE_SM_MMSE, N_SS > 1) returns
 * DNRP_EUNSUPPORTED before anything is launched. DNRP_EINVAL for a NULL context, on > 1, a non-finite gain or
 * a gain outside [0, 1]; a refused call changes nothing. The getter's outputs may be NULL.
 *
 * dnrp_rx_sto_track: stream-ordered copy of the increment every OFDM symbol was derotated with by the latest
 * dnrp_rx_pcc_batch / dnrp_rx_pdc_batch: inc is a host array [n_slots][*n_sym], slot = index in the PCC batch,
 * *n_sym = symbols the PCC call's windows hold + 1. Symbol 0 holds the STF estimate, symbols that were not
 * processed (behind the PCC phase of a packet no PDC request continued, behind a packet's end) hold NaN.
 * inc NULL: only *n_sym is written (size query). Valid once `stream` has been synchronised.
 * DNRP_EINVAL while the latest PCC call ran with tracking off or there was none, for n_slots = 0 or beyond
 * that call's n, or n_sym_cap < *n_sym.
 */
int dnrp_ctx_set_rx_sto_tracking(dnrp_ctx* ctx, uint32_t on, float gain);
int dnrp_ctx_get_rx_sto_tracking(const dnrp_ctx* ctx, uint32_t* on, float* gain);
int dnrp_rx_sto_track(dnrp_ctx* ctx, uint32_t n_slots, double* inc, uint32_t n_sym_cap, uint32_t* n_sym, void* stream);

/*
 * Residual CFO tracking from the DRS symbols <- the intent of the build option
 * RX_SYNCED_PARAM_CFO_RESIDUAL_BASED_ON_DRS (rx_synced_param.hpp:162-181: "two OFDM symbols with DRS cells are
 * compared, their spacing in time domain is N_step"; rx_synced.cpp:843-852), which the reference comments out
 * as not functional: its estimator_cfo.cpp:65-74 multiplies neighbouring cells of one symbol, which measures a
 * timing slope. The sister of dnrp_ctx_set_rx_sto_tracking: carrier and sampling clock share one oscillator.
 *   on  0 (default): exactly the receiver without the option: every data-field symbol of a packet is mixed
 *       with the increment the STF refined, the same launches, byte-identical LLRs and reports.
 *       1: after every DRS symbol l that has an earlier DRS symbol l' of the same transmit streams, the rotation
 *       between the two -- the angle of C = sum h_l[i] conj(h_l'[i]) + h_l[i] conj(h_l'[i -+ 1]) over the
 *       zero-forced pilots i, the streams TS_first..min(TS_last, 7) and the RX antennas, the two cells of l'
 *       being those on either side of cell i, so that a timing offset cancels to first order -- less what the
 *       table has already removed, divided by (l - l') (CP + N_b_DFT_os) samples and times `gain`, is taken off
 *       the mixer increment of every later symbol; the mixer phase stays continuous at the first CP sample of
 *       symbol l + 1 (mixer.cpp adjust_phase_increment). A DRS symbol itself is mixed with the values from before
 *       its own update. The PDC phase continues from the PCC phase's state. The fused receiver
 *       (DNRP_RX_FUSED) and the grouped Y path (DNRP_RX_GROUP) are not taken while it is on. It may be on
 *       together with STO tracking: both measure the same rows, front-ended with the STF values alone.
 *   gain  scales each residual: 0 runs the whole mechanism with every symbol's entry equal to the STF values
 *       (LLRs byte-identical to off).
 * Read once per dnrp_rx_pcc_batch; that call's dnrp_rx_pdc_batch takes the same values. With it on, a
 * dnrp_rx_pdc_batch request for spatial multiplexing returns DNRP_EUNSUPPORTED before anything is launched.
 * DNRP_EINVAL for a NULL context, on > 1, a non-finite gain or a gain outside [0, 1]; a refused call changes
 * nothing. The getter's outputs may be NULL.
 *
 * dnrp_rx_cfo_track: stream-ordered copy of the mixer entry every OFDM symbol was mixed with by the latest
 * dnrp_rx_pcc_batch / dnrp_rx_pdc_batch: inc and phase are host arrays [n_slots][*n_sym] (either may be NULL),
 * slot = index in the PCC batch, *n_sym = symbols the PCC call's windows hold + 1. The mixer phase of DECT-rate
 * sample m of symbol l (counted from the packet's first sample, CP included) is
 * phase[l] + (m - n_stf) inc[l], n_stf = STF_CP + N_b_DFT_os samples; without an update the entry is
 * (n_stf inc0, inc1), the sync report's increment and the STF's. Symbols that were not processed hold NaN.
 * inc and phase NULL: only *n_sym is written (size query). Valid once `stream` has been synchronised.
 * DNRP_EINVAL while the latest PCC call ran with tracking off or there was none, for n_slots = 0 or beyond
 * that call's n, or n_sym_cap < *n_sym.
 */
int dnrp_ctx_set_rx_cfo_tracking(dnrp_ctx* ctx, uint32_t on, float gain);
int dnrp_ctx_get_rx_cfo_tracking(const dnrp_ctx* ctx, uint32_t* on, float* gain);
int dnrp_rx_cfo_track(dnrp_ctx* ctx, uint32_t n_slots, double* inc, double* phase, uint32_t n_sym_cap, uint32_t* n_sym,
                      void* stream);

/*
 * MIMO report options <- the build options RX_SYNCED_PARAM_MODE_3_7_METRIC and
 * RX_SYNCED_PARAM_MIMO_USE_ALL_W_MATRICES_OR_ONLY_NON_ZERO (lib/include/dectnrp/phy/rx/rx_synced/
 * rx_synced_param.hpp:273-286; estimator_mimo.cpp:162-271), a read-back of the report's inputs and scores, and
 * the rank / precoder report for spatial multiplexing that mimo_report_t declares (RI, PMI, mimo_report.hpp:51-58)
 * and the reference never fills.
 *   metric  how the codebook search of tm_3_7_beamforming_idx / _reciprocal_idx combines, per candidate, the
 *           receive side's |sum_tx sum_c H w| (float, the reference's order):
 *           DNRP_MIMO_METRIC_HIGHEST_MIN_RX_POWER (default) their minimum, the largest wins (from -1e6);
 *           DNRP_MIMO_METRIC_MAX_RX_POWER their sum in ascending antenna order, the largest wins (from -1e6);
 *           DNRP_MIMO_METRIC_MIN_SPREAD_RX_POWER maximum - minimum, the smallest wins (from +1e6).
 *           The combination is multiplied by the entry's scaling factor (the reference's comment says
 *           "ignoring", its code multiplies). The first candidate in index order wins a tie.
 *   all_w   0 (default): the search starts at the first entry without a zero element (2 for 2 antennas, 12 for
 *           4); 1: at entry 0.
 *   detail  1: every later dnrp_rx_pdc_batch keeps one dnrp_mimo_detail per request (also without `rep`).
 * (0, 0, 0) is exactly the receiver without the options: rx_mimo_kernel, launched only where the caller passes
 * `rep`, the same reports, no further launch, allocation or copy. Under any other setting
 * rx_mimo_detail_kernel runs in its place for every request (timer "rx_mimo_detail"); with metric 0 and all_w 0
 * it computes the same indices with the same arithmetic in the same order. Read once per dnrp_rx_pdc_batch; a
 * retained PCC batch stays valid. Every PDC path (plain Y, grouped Y, epoch, fused) stays selectable: each runs
 * rx_snr_kernel over all DRS ops of the phase, which leaves the noise variance the report reads. DNRP_EINVAL
 * for a NULL context, metric > 2, all_w > 1 or detail > 1; a refused call changes nothing. The getter's
 * outputs may be NULL.
 *
 * dnrp_mimo_detail (the extension is marked *):
 *   H         the stage: the latest zero-forced DRS value of every (rx, transmit stream) at the 4 wideband
 *             cells, as the search reads it
 *   nv        the SNR chain's noise variance per RX cell after the packet's last DRS symbol (the value the MMSE
 *             receiver of DNRP_RX_MODE_SM_MMSE regularises with); nv_used* = max(nv, 2^-14 P, FLT_MIN), P the
 *             mean |H|^2 of the stage: a noise-free packet stays finite, the SINR is capped near 42 dB
 *   idx_*     the report's two indices; score_*: metric times scaling of every scored index, NaN elsewhere. A
 *             side with one antenna reports index 0 and no score, one with 8 antennas (no single-stream
 *             codebook) 0xFFFFFFFF and no score
 *   rate_cb*  [s][cb]: rank slot s = 0, 1, 2 stands for R = 1, 2, 4 layers, available iff R <= min(N_TS, N_RX)
 *             and N_TS in {1, 2, 4} (codebook (R, N_TS) of W_t; none at N_TS = 8). Per wideband cell c, He =
 *             H_c W_cb scaling_cb (N_RX x R), G = He^H He + nv_used I, r_c = sum_i -log2(nv_used [G^-1]_ii), the
 *             sum over the layers of log2(1 + MMSE SINR); rate_cb = (r_0 + r_1 + r_2 + r_3) / 4 bits per cell
 *   pmi*, rate*  the first maximum of rate_cb[s] and its rate; RI*: the R with the largest rate (a tie goes to
 *             the lower rank), PMI* = pmi[slot of RI]; sinr_eff_dB* = 10 log10(2^(rate[RI] / RI) - 1), the
 *             number a caller maps to an MCS (no CQI: the reference has no SINR-to-MCS table)
 * dnrp_rx_mimo_detail: stream-ordered copy of rows 0..m-1 of the latest dnrp_rx_pdc_batch, in request order,
 * valid once `stream` has been synchronised. DNRP_ESTATE if that call did not run with detail = 1 or there was
 * none; DNRP_EINVAL for NULL pointers, m = 0 or m above that call's m.
 */
#define DNRP_MIMO_METRIC_HIGHEST_MIN_RX_POWER 0u
#define DNRP_MIMO_METRIC_MAX_RX_POWER 1u
#define DNRP_MIMO_METRIC_MIN_SPREAD_RX_POWER 2u
#define DNRP_MIMO_MAX_CB 28u /* largest codebook of W_t: (N_SS 1, N_TX 4) */

int dnrp_ctx_set_rx_mimo_report(dnrp_ctx* ctx, uint32_t metric, uint32_t all_w, uint32_t detail);
int dnrp_ctx_get_rx_mimo_report(const dnrp_ctx* ctx, uint32_t* metric, uint32_t* all_w, uint32_t* detail);

typedef struct {
    uint32_t N_RX, N_TS;
    float H[8][8][4][2];      /* [rx][ts][wideband cell] (re, im), zero beyond N_RX / N_TS */
    float nv, nv_used;
    uint32_t idx_tx, idx_rx;  /* = tm_3_7_beamforming_idx / _reciprocal_idx of the report */
    float score_tx[DNRP_MIMO_MAX_CB], score_rx[DNRP_MIMO_MAX_CB];
    uint32_t RI, PMI;         /* rank in {1, 2, 4} and its codebook index; 0 / 0xFFFFFFFF: none */
    uint32_t pmi[3];          /* best codebook index per rank slot (R = 1, 2, 4), 0xFFFFFFFF: rank not available */
    float rate[3];            /* its rate in bits per cell, NaN: not available */
    float rate_cb[3][DNRP_MIMO_MAX_CB]; /* every candidate's rate, NaN where there is none */
    float sinr_eff_dB;
} dnrp_mimo_detail;

int dnrp_rx_mimo_detail(dnrp_ctx* ctx, uint32_t m, dnrp_mimo_detail* out, void* stream);

/*
 * Angle-of-arrival report from the DRS pilots <- estimator_aoa_t (lib/include/dectnrp/phy/rx/rx_synced/aoa/
 * estimator_aoa.hpp; rx_synced.cpp:133, 251), whose reset / process_stf / process_drs bodies are empty in the
 * reference. The estimator is this project's own:
 *   R[a][b] = sum h_a conj(h_b) over every DRS cell of every transmit stream of every DRS symbol of the packet
 *             (the PCC phase's included), h_a the zero-forced pilot w y of RX antenna a. Whatever is common to
 *             the antennas (CFO mixing, STO derotation, residual tracking, the amplitude scale) cancels.
 *             Products in float, sums across lanes and DRS symbols in double in a fixed order (bit-identical
 *             from run to run), stored as float; R[b][a] = conj(R[a][b]) exactly, the diagonal's imaginary
 *             parts exactly 0, rows and columns at index >= N_RX zero. n_cells: cells summed per antenna.
 *   array     antenna r at pos[r] = (x_r, y_r) in carrier wavelengths; steering vector a_r(az) =
 *             exp(j 2 pi (x_r cos az + y_r sin az)). Narrowband: one wavelength for the whole occupied band
 *             (at most 1.5 % of the carrier). Entries of pos at index >= N_RX are not used but must be finite.
 *   scan      Bartlett: P(g) = a(az_g)^H R a(az_g) / (N_RX tr R) on n_grid azimuths, az_g = az_min + g step,
 *             step = (az_max - az_min) / (n_grid - 1), end points included; where az_max - az_min is 2 pi (within
 *             1e-5, the rounding of the float end points) the grid is cyclic, step = 2 pi / n_grid, without the
 *             end point. The steering table is computed in double on the host when the setting is made; the
 *             quadratic form runs in double on the device from R as stored. grid_idx: the first maximum
 *             (strictly greater, from 0). az_rad / peak: the vertex of the parabola through the maximum and its
 *             two neighbours (wrapping on a cyclic grid, az_rad brought back to >= az_min there); the grid point
 *             itself at an end point of a non-cyclic grid. tr R = 0: az_rad = 0, peak = 0, grid_idx = 0xFFFFFFFF.
 *   lag       lag_re + j lag_im = sum_a R[a + 1][a]: for a uniform line of spacing d along y its argument is
 *             2 pi d sin az, the caller takes asin(arg / (2 pi d)).
 * dnrp_ctx_set_rx_aoa: cfg NULL = off (the default: no launch, allocation or copy, LLRs and reports byte for
 * byte as before). On, every later dnrp_rx_pdc_batch runs rx_aoa_kernel (timer "rx_aoa") for every request, with
 * or without `rep`; the fused PDC receiver is not chosen (its DRS bins are not in Y), every other path and the
 * MMSE receiver stay selectable. Read once per dnrp_rx_pdc_batch: a call in flight keeps the setting it read.
 * DNRP_EINVAL for a NULL context, a context with N_TX_max < 2, non-finite values, n_grid outside 8..512,
 * az_max <= az_min, az_max - az_min > 2 pi (+ 1e-5) or reserved != 0; a refused call changes nothing.
 * dnrp_ctx_get_rx_aoa: *on and, where on, *cfg (either may be NULL).
 * dnrp_rx_aoa: stream-ordered copy of rows 0..m-1 of the latest dnrp_rx_pdc_batch, in request order, valid once
 * `stream` has been synchronised. DNRP_ESTATE if that call did not run the kernel or there was none;
 * DNRP_EINVAL for NULL pointers, m = 0 or m above that call's m.
 * dnrp_aoa_estimate: host only, no context or device: everything of *out but R and n_cells (left as they are)
 * from R [8][8][2] floats (re, im; the layout of dnrp_aoa_report::R) for N_RX in 2..8 antennas, by the code
 * that builds the table the setter uploads and the scan code the kernel runs; spectrum: NULL or [n_grid], P(g)
 * (all 0 where tr R = 0). DNRP_EINVAL for NULL cfg / R / out, N_RX outside 2..8 or a cfg the setter refuses.
 */
typedef struct {
    float pos[8][2];          /* (x, y) of every RX antenna in carrier wavelengths */
    float az_min, az_max;     /* rad */
    uint32_t n_grid;          /* 8..512 */
    uint32_t reserved;        /* 0 */
} dnrp_aoa_cfg;

typedef struct {
    float R[8][8][2];         /* [a][b] (re, im) */
    uint32_t n_cells, grid_idx;
    float az_rad, peak, lag_re, lag_im;
    uint32_t reserved[2];
} dnrp_aoa_report;

int dnrp_ctx_set_rx_aoa(dnrp_ctx* ctx, const dnrp_aoa_cfg* cfg);
int dnrp_ctx_get_rx_aoa(const dnrp_ctx* ctx, uint32_t* on, dnrp_aoa_cfg* cfg);
int dnrp_rx_aoa(dnrp_ctx* ctx, uint32_t m, dnrp_aoa_report* out, void* stream);
int dnrp_aoa_estimate(const dnrp_aoa_cfg* cfg, uint32_t N_RX, const float* R, dnrp_aoa_report* out, float* spectrum);

/*
 * Ring-buffer window gather <- rx_pacer_t's wrap copy (rx_pacer.cpp:106-143) over the per-antenna
 * ring of radio::buffer_rx_t (radio/buffer_rx.hpp:46-141; sample of global time t at index
 * t % ring_len). Copies window w = global samples [start[w], start[w] + S_win) of antennas
 * 0..N_ant-1 into out [n][N_ant][S_win] cf32 (device), ready for dnrp_rx_sync_batch or the RX.
 *   ring   device cf32, antenna a at ring + 2*a*ant_stride floats (ant_stride >= ring_len)
 *   start  host [n], >= 0; S_win <= ring_len (one wrap at most); n * N_ant <= 65535
 */
int dnrp_ring_gather(dnrp_ctx* ctx, const float* ring, uint64_t ring_len, uint64_t ant_stride, uint32_t N_ant,
                     uint32_t n, const int64_t* start, uint32_t S_win, float* out, void* stream);

/* Continuous-stream synchronisation state = baton_t's uniqueness state (baton.cpp:37-52,157-169):
 * the latest unique fine peak time and the minimum distance to it (worker_pool.cpp:299-321) */
typedef struct {
    int64_t sync_time_last;          /* global hw time of the latest unique packet */
    int64_t sync_time_unique_limit;  /* one STF pattern at b * os_min (..._UNIQUE_LIMIT_IN_STF_PATTERNS_DP) */
    uint64_t packets, not_unique;    /* worker_sync_t stats: job_packet, job_packet_not_unique */
} dnrp_sync_stream_state;

int dnrp_sync_stream_init(const dnrp_ctx* ctx, const dnrp_sync_cfg* sc, dnrp_sync_stream_state* state);

/* hw samples one chunk's search reads from the ring: chunk_len plus the detection overlap into the
 * next chunk, the coarse-peak and cross-correlation spans and the resampler filter (sync_chunk.cpp:
 * 32-123); 0 on a bad argument. Must be <= the ring length. */
uint32_t dnrp_sync_stream_window(const dnrp_ctx* ctx, const dnrp_sync_cfg* sc);

/*
 * Continuous-stream synchronisation <- the sync worker pool (worker_sync_t::work,
 * worker_sync.cpp:57-221) over n_chunks consecutive chunks of sc->chunk_len hw samples starting at
 * global time t0: every chunk's window is gathered from the ring, searched with
 * sync_chunk_t::search() (up to sc->max_reports packets per chunk), its reports converted to global
 * time (coarse_peak_time / fine_peak_time, sync_chunk.cpp:213-245) and passed through the baton's
 * double-detection filter in chunk order (baton.cpp:157-169: unique iff fine_peak_time - last >
 * limit). out (host, n_chunks * max_reports) receives the unique reports in time order, n_out their
 * count, chunk_of (host, optional) the chunk each was found in. Blocking: returns after the stream's
 * work has completed. Call again with t0 advanced by n_chunks * chunk_len to continue the stream.
 */
int dnrp_rx_sync_stream(dnrp_ctx* ctx, const dnrp_sync_cfg* sc, const float* ring, uint64_t ring_len,
                        uint64_t ant_stride, int64_t t0, uint32_t n_chunks, dnrp_sync_stream_state* state,
                        dnrp_sync_result* out, uint32_t* n_out, uint32_t* chunk_of, void* stream);

/*
 * Simulated wireless channel <- the virtual space links of the reference's simulator
 * (lib/src/simulation/wireless/channel_awgn.cpp, channel_flat.cpp, channel_doubly.cpp + link.cpp;
 * noise: lib/src/simulation/hardware/noise.cpp). Applies N_TX x N_RX links to n TX windows:
 *   awgn    every TX antenna superimposed onto every RX antenna (large-scale factor only)
 *   flat    one Rayleigh coefficient per link and window
 *   doubly  tapped delay line per link: a 3GPP power delay profile (link.hpp:88-108, pdp_idx 0..2 =
 *           EPA / EVA / ETU) scaled to tau_rms_ns, 40 Doppler sinusoids per tap (Jakes, fD_Hz)
 * then complex AWGN with n0 = -10 log10(net_bw_norm) - snr_db dB (per unit signal power in the net
 * bandwidth; snr_db >= DNRP_CH_NOISELESS_DB: none). Link realisations are drawn per window from the
 * seed (window index within the call); dnrp_channel_realization returns them (host only).
 *   tx      device [n][N_TX][S_tx] cf32; rx device [n][N_RX][S_rx] cf32 (every sample written)
 *   offset  host [n]: TX sample 0 lands at RX sample offset[w] (zero input outside [0, S_tx))
 *   t0      host [n]: global hw time of RX sample 0 (phases of the Doppler sinusoids)
 */
#define DNRP_CH_AWGN 0
#define DNRP_CH_FLAT 1
#define DNRP_CH_DOUBLY 2
#define DNRP_CH_NOISELESS_DB 1000.0f
typedef struct {
    uint32_t kind;          /* DNRP_CH_* */
    uint32_t pdp_idx;       /* doubly: power delay profile 0..2 */
    float tau_rms_ns;       /* doubly: delay spread, <= 2000 */
    float fD_Hz;            /* doubly: maximum Doppler, <= 2000 */
    uint32_t samp_rate;     /* hw sample rate in S/s (tap delays, Doppler periods) */
    float large_scale;      /* amplitude factor of every link (path loss / RX sensitivity) */
    float snr_db;           /* noise level, see above */
    float net_bw_norm;      /* N_b_OCC / N_b_DFT_os scaled to the hw rate (noise.cpp net_bandwidth_norm) */
    uint64_t seed;
} dnrp_channel_cfg;

int dnrp_channel_batch(dnrp_ctx* ctx, const dnrp_channel_cfg* cfg, uint32_t n, uint32_t N_TX, const float* tx,
                       uint32_t S_tx, uint32_t N_RX, const int64_t* offset, const int64_t* t0, float* rx, uint32_t S_rx,
                       void* stream);
/* Host only: window w's realisation. n_taps receives the taps per link (doubly); arrays (optional)
 * are [N_RX][N_TX][n_taps] delay (samples) / amp, [N_RX][N_TX][n_taps][40] period / phase_rev
 * (initial phase in revolutions), [N_RX][N_TX][2] coef (flat). */
int dnrp_channel_realization(const dnrp_channel_cfg* cfg, uint32_t window, uint32_t N_TX, uint32_t N_RX, uint32_t* n_taps,
                             int32_t* delay, float* amp, int64_t* period, double* phase_rev, float* coef);

/*
 * Virtual space <- vspace_t::wchannel_execute (lib/src/simulation/vspace.cpp:449-513) followed by the
 * simulated radio's clip_and_quantize (lib/src/radio/hw_simulator.cpp:686-733): the emissions of all
 * devices, each through its own link, superimposed into one receiver's ring (the buffer_rx_t layout
 * dnrp_ring_gather and dnrp_rx_sync_stream read: sample of global time t at index t % ring_len).
 */
/* One transmission as the receiver sees it (vspptx_t: tx_idx / tx_length and its samples, vspace.cpp:457-487) */
typedef struct {
    int64_t  t_start;   /* global hw time at which TX sample 0 of this emission reaches the receiver */
    uint32_t tx_row;    /* row of tx [n_rows][N_TX][S_tx] holding its samples (a dnrp_tx_batch row) */
    uint32_t length;    /* samples on the air, 1..S_tx (dnrp_tx_transmit_length) */
    uint32_t link;      /* link realisation: dnrp_channel_realization(cfg, window = link); emissions of one
                           device pair share it (the edge index of vspace.cpp:463-468) */
    uint32_t own;       /* 1: the receiver's own transmission (vspace.cpp:471-487) */
    float    gain;      /* amplitude factor of this emission's links, times cfg->large_scale
                           (channel.cpp:53-73: db2mag(tx power - path loss or leakage - rx power)); >= 0 */
    uint32_t reserved;  /* 0 */
} dnrp_vspace_emission;   /* 32 bytes */

/* The simulated ADC (hw_simulator_t::clip_and_quantize, hw_simulator.cpp:710-733) */
typedef struct {
    float    clip_limit; /* > 0: re and im clamped to +-clip_limit (clip.cpp); 0: samples pass unchanged */
    uint32_t n_bits;     /* > 0 (with clip_limit > 0): re and im rounded to multiples of
                            2*clip_limit / 2^n_bits, roundf (quantize.cpp, hw_simulator.cpp:710-733); <= 24 */
} dnrp_adc_cfg;

/*
 * For every global time t in [t_begin, t_begin + n_samples) and every antenna r < N_RX the ring sample
 * at ring + 2*(r*ant_stride + t % ring_len) floats is written exactly once; nothing is read from the
 * ring and no other ring sample is touched. Its value (vspace.cpp:453-498, then the ADC):
 *   s_r(t)  = sum over emissions e with own == 0, in em[] order, of gain_e * large_scale * link_e(r, x_e, t - t_start_e)
 *   s_r(t)  = 0 where any own emission has t in [t_start, t_start + length)   (RX detached, vspace.cpp:477-479)
 *   s_r(t) += the own emissions through their links with their gain           (leakage, vspace.cpp:487; gain 0: none)
 *   y_r(t)  = s_r(t) + sigma * z_r(t)                                         ("relative" noise, vspace.cpp:489-498)
 *   ring    = adc(y_r(t))          (clamp first, then roundf(y / bit_width) * bit_width; adc NULL: y_r(t))
 * link_e is dnrp_channel_batch's per-sample link (awgn / flat / doubly of cfg->kind) with the realisation
 * of index em[e].link; TX samples outside [0, length) are zero, the Doppler phases come from the global
 * t, and with the doubly kind an emission reaches its largest tap delay past its length. sigma is
 * dnrp_channel_batch's noise level; z_r(t) comes from a counter-based generator keyed by (seed, r, all
 * 64 bits of t).
 * Split invariance: a sample's value depends on its global time alone, never on t_begin, n_samples or
 * how the span was tiled. Any split of a span over several calls with the same em[] therefore leaves
 * bit-identical ring contents to one call over the whole span: a caller may fill the ring in
 * instalments while dnrp_rx_sync_stream follows behind.
 * An emission wholly outside the span is ignored; one that begins before it or ends after it
 * contributes the part inside. Stream-ordered and non-blocking, like dnrp_channel_batch; n_samples == 0
 * does nothing.
 *   tx      device [n_rows][N_TX][S_tx] cf32 (em and tx may be NULL when n_em == 0: noise only)
 *   ring    device cf32, antenna r at ring + 2*r*ant_stride floats; ant_stride >= ring_len >= n_samples
 *   DNRP_EINVAL: a null pointer, N_TX / N_RX outside 1..8, t_begin or a t_start < 0, length outside
 *   1..S_tx, tx_row >= n_rows, a negative or non-finite gain, reserved != 0, clip_limit < 0,
 *   n_bits > 24, a configuration dnrp_channel_batch refuses.
 */
int dnrp_vspace_mix(dnrp_ctx* ctx, const dnrp_channel_cfg* ch, const dnrp_adc_cfg* adc /* NULL = none */,
                    uint32_t n_em, const dnrp_vspace_emission* em, uint32_t N_TX, const float* tx,
                    uint32_t n_rows, uint32_t S_tx, uint32_t N_RX, float* ring, uint64_t ring_len,
                    uint64_t ant_stride, int64_t t_begin, uint64_t n_samples, void* stream);

/* One channel measurement <- chscan_t (lib/include/dectnrp/phy/rx/chscan/chscan.hpp) */
typedef struct {
    int64_t  end;        /* global hw time of the final sample scanned (chscan_t::end_64) */
    uint32_t length;     /* samples per partial scan, >= 2 (duration_lut of chscan_t::duration_ec, above this boundary) */
    uint32_t N_partial;  /* partial scans, >= 1 */
    uint32_t N_ant;      /* antennas used, clamped to the ring's N_ant (chscanner.cpp:44) */
    uint32_t reserved;
} dnrp_chscan_req;

/*
 * Channel scanner <- chscanner_t::scan for n requests at once (lib/src/phy/rx/chscan/chscanner.cpp:38-141)
 * over the ring dnrp_ring_gather reads: start = end - (N_partial*length - 1), partial scan p covers global
 * samples [start + p*length, start + (p+1)*length) with the ring's wrap, and its value
 * sqrt(energy over the used antennas / (length * N_ant_used)) goes to rms_partial[partial_offset[i] + p]
 * (host). rms_avg[i] (host) is what scan() leaves in chscan_t::rms_avg: the SUM of the partial values
 * -- scan() adds them and never divides (chscanner.cpp:63-74), so a caller porting get_rms_avg() sees
 * the same number. The square roots are taken on the device, the sums on the host after the copy.
 * Blocking: returns after the stream's work has completed, the host arrays are then valid.
 *   DNRP_EINVAL: a null pointer, length < 2 (scan_partial's A < B test mistakes a one-sample span for a
 *   wrap), N_partial == 0, N_ant == 0, start < 0, N_partial*length > ring_len.
 */
int dnrp_chscan_batch(dnrp_ctx* ctx, const float* ring, uint64_t ring_len, uint64_t ant_stride, uint32_t N_ant,
                      uint32_t n, const dnrp_chscan_req* req, float* rms_partial, const uint32_t* partial_offset,
                      float* rms_avg, void* stream);

/* Host only. N_samples_transmit_os_rs: the samples a radio buffer holds once the packet is complete
 * (packet without GI + GI_percentage % of the GI, tx.cpp:555-566) = the final value of the
 * reference's progressive buffer_tx_t::set_tx_length_samples_cnt (tx.cpp:241,277,292). dnrp_tx_batch
 * completes every buffer before its stream work completes; samples past this length are zero. */
int dnrp_tx_transmit_length(const dnrp_cfg* cfg, const dnrp_psdef* psdef, uint32_t GI_percentage, uint32_t* len);

/* Host only: JSON export in the reference's formats.
 *   dnrp_tx_packet_json <- tx_t::write_all_data_to_json (tx.cpp:316-427): packet definition, TX
 *     meta, d-bits of PCC and PDC (PLCF / TB fields empty: they sit above the FEC), the antenna
 *     streams (host copy of dnrp_tx_batch's iq_out row, [N_TX][S] cf32) up to the transmit length,
 *     resampler parameters.
 *   dnrp_rx_packet_json <- worker_tx_rx_t::collect_and_write_json's RADIO/PHY part
 *     (worker_tx_rx.cpp:354-396; rx_synced's channel estimates are not exported). */
int dnrp_tx_packet_json(const dnrp_cfg* cfg, const dnrp_psdef* psdef, const dnrp_tx_desc* desc, uint32_t rv,
                        uint64_t tx_order_id, int64_t tx_time_64, const uint8_t* pcc_d, const uint8_t* pdc_d,
                        const float* iq, uint32_t S, const char* path);
int dnrp_rx_packet_json(const dnrp_cfg* cfg, uint32_t worker_id, const dnrp_sync_result* sr, uint32_t mcs_index,
                        const dnrp_pcc_report* pcc, const dnrp_pdc_report* pdc, const char* path);

/* sp3::radio_device_class_t (sections_part3/radio_device_class.hpp): the capabilities of a device
 * class string such as "8.16.8.A"; a worker pool sizes itself from them (dnrp_cfg.u_max = u_min,
 * b_max = b_min, N_TX_max = N_TX_min, as worker_pool_config_t does). Host only. DNRP_ECONFIG for a
 * class the reference does not list (radio_device_class.cpp:26-150). */
typedef struct {
    uint32_t u_min, b_min, N_TX_min, mcs_index_min, M_DL_HARQ_min, M_connection_DL_HARQ_min, N_soft_min, Z_min;
    uint32_t PacketLength_min;
} dnrp_radio_device_class;
int dnrp_get_radio_device_class(const char* name, dnrp_radio_device_class* out);

/* The reference parameters the library is built with, by the reference's own names (sync_param.hpp
 * RX_SYNC_PARAM_*, rx_synced_param.hpp RX_SYNCED_PARAM_* incl. "NAME[i]" vector entries, flags as
 * 1 = defined / 0 = not defined, resampler_param_t::f_pass_norm[user][os] etc., constants::*).
 * Host only: DNRP_EINVAL for an unknown name. dnrp_param_name(i) enumerates them (NULL past the end). */
int dnrp_query_param(const char* name, double* value);
const char* dnrp_param_name(uint32_t index);
/* The literal tables of sections_part3 the library builds its device tables from (host only), for
 * pinning against the reference's own text (tests/golden/ref_literals.json). Returns the number of
 * floats (out may be NULL to ask for it; cap = floats available), DNRP_EINVAL for an unknown name or
 * bad arguments. Names (arguments):
 *   "W" (N_TS, N_TX, codebook)   W_t matrix [N_TX][N_TS] re/im (Tables 6.3.4-1..6)
 *   "W_scaling" / "W_scaling_optimal_DAC" (N_TS, N_TX, codebook)   its scaling factor (tx.cpp:582-592)
 *   "W_codebooks" (N_TS, N_TX)   number of codebook entries
 *   "stf" (b, N_eff_TX)          stf_t transmit-stream vector [N_b_OCC + 1] re/im, scale 1 (stf.cpp:185-285)
 *   "drs_values" (b, t)          the N_b_OCC/4 DRS values of transmit stream t (drs.cpp:227-254)
 *   "txdiv_pairs" (N_TS)         Y_i_t::index_N_TS_x rows A0 B0 A1 B1 ... (transmit_diversity_precoding.cpp:48-75)
 *   "stf_cover_sequence" ()      stf_t::cover_sequence (stf.hpp:146-151)
 *   "cells_lds_bytes" (u_max, b_max, b, N_RX, N_eff_TX)   LDS bytes of the PDC equaliser's staging for
 *                                the geometry; above 160 KiB dnrp_rx_*_batch return DNRP_EUNSUPPORTED
 *   "fused_lds_bytes" (N_RX)     LDS bytes of a fused PDC receiver launch (DNRP_RX_FUSED=1); above 160 KiB the
 *                                PDC phase takes another receiver
 *   "symbol_cells" (b, N_TS, N_eff_TX, N_DF)   per symbol l = 0..N_DF the number of PCC, PDC and DRS cells
 *   "pdc_cells" (b, N_TS, N_eff_TX, N_DF)   per PDC cell in mapping order: symbol l, subcarrier index k
 *                                (pdc.cpp:108-153; k counts from the lowest occupied subcarrier, DC included)
 *   "pcc_cells" (b, N_TS)        per PCC cell in mapping order: symbol l, subcarrier index k (pcc.cpp:83-108)
 *   "drs_cells" (b, N_TS, N_DF)  per DRS symbol: l, ts_first, ts_last, then the N_b_OCC/4 subcarrier
 *                                indices k of each transmit stream ts_first..ts_last (drs.cpp:73-125)
 *   "rx_epoch_syms" (b, N_TS, N_eff_TX, N_DF, mode_lr, stride)   the epoch receiver's symbol ownership of
 *                                the PDC phase: ok (0 / 1), per plan epoch its symbol count and symbols,
 *                                then the DRS-pass symbols
 *   "sync_template" (u, b_max, os_min, L, M, b, N_eff_TX)   the fine search's time-domain STF template of a b
 *                                packet in the stream of a (u, b_max, os_min, L, M) receiver: tmpl_len =
 *                                stf_len L / M hw samples re/im (stf_template.cpp:93-199; the row of b = b_max
 *                                is the one searched without dnrp_ctx_set_sync_beta_search). DNRP_EINVAL for
 *                                b > b_max, a b outside {1, 2, 4, 8, 12, 16} or an N_eff_TX outside {1, 2, 4, 8} */
int dnrp_query_table(const char* name, const uint32_t* arg, uint32_t n_arg, float* out, uint32_t cap);

/* Kernel timing (only when the environment has DNRP_TIMING=1 at dnrp_ctx_create): HIP events
 * recorded on the caller's stream around each launch. Names: "tx", "sync_steps", "sync_detect",
 * "sync_post", "sync_fine", "rx_stf", "rx_fft_pcc", "rx_pcc", "rx_fft_pdc", "rx_pdc", "vspace_mix", "chscan". */
int dnrp_last_kernel_ms(const dnrp_ctx* ctx, const char* name, float* ms);
int dnrp_kernel_time_total(dnrp_ctx* ctx, const char* name, float* total_ms, uint32_t* count, int reset);

/*
 * Channel coding (host only) <- phy/fec/fec.cpp (fec_t), pcc_enc.cpp, pdc_enc.cpp and
 * sections_part3/fix/cbsegm.cpp: CRC attachment, code-block segmentation, LTE turbo code (TS 36.212
 * §5.1.3, QPP interleaver), turbo rate matching (§5.1.4.1) and a max-log-MAP turbo decoder with
 * CRC early stopping. The split with the GPU path is the reference's scrambler: the encoders output
 * the rate-matched d-bits dnrp_tx_batch takes (pcc_d / pdc_d: unscrambled, MSB first) and the
 * decoders take the descrambled int16 LLRs dnrp_rx_pcc_batch / dnrp_rx_pdc_batch return.
 */
#define DNRP_CRC16 0   /* PLCF CRC, g = 0x1021 (pcc_enc.cpp:88-91) */
#define DNRP_CRC24A 1  /* transport-block CRC, g = 0x864CFB (pdc_enc.cpp:60-63) */
#define DNRP_CRC24B 2  /* code-block CRC, g = 0x800063 (pdc_enc.cpp:56-59) */

/* srsran_cbsegm_t as filled by srsran_cbsegm_FIX (cbsegm.cpp:65-123): C2 blocks of K2 first */
typedef struct {
    uint32_t tbs, Z, C, C1, C2, K1, K2, K1_idx, K2_idx, F;
} dnrp_cbsegm;

/* sp3::fec_cfg_t (sections_part3/derivative/fec_cfg.hpp). PLCF_type and network_id select the
 * scrambling sequence, which the GPU path applies: they are carried for the mirror only. */
typedef struct {
    uint32_t PLCF_type, closed_loop, beamforming, N_TB_bits, N_bps, rv, G, network_id, Z;
} dnrp_fec_cfg;

/* HARQ RX softbuffer (harq::buffer_rx_t): accumulated code-block softbits, code-block CRC flags
 * and the code blocks already decoded, kept across redundancy versions of one transport block. */
typedef struct dnrp_harq_rx dnrp_harq_rx;

int dnrp_crc(const uint8_t* data, uint32_t nbits, uint32_t kind, uint32_t* crc);
int dnrp_fec_cbsegm(uint32_t N_TB_bits, uint32_t Z, dnrp_cbsegm* out);
/* row idx (0..187) of TS 36.212 Table 5.1.3-3: K and the QPP coefficients f1, f2 (optional) */
int dnrp_fec_cb_size(uint32_t idx, uint32_t* K, uint32_t* f1, uint32_t* f2);

/* fec_t::encode_plcf without the scrambling: plcf (5 or 10 bytes) -> d [25] bytes (196 bits).
 * closed_loop / beamforming select the CRC mask (pcc_enc.cpp:170-183). */
int dnrp_pcc_encode(const uint8_t* plcf, uint32_t plcf_type, uint32_t closed_loop, uint32_t beamforming, uint8_t* d);
/* fec_t::decode_plcf_test after the descrambling: llr [196] -> 1 if a PLCF of plcf_type_test passed
 * its CRC under one of the four masks (plcf [5 or 10], closed_loop, beamforming set), 0 if not.
 * Up to 5 turbo iterations, stopping at the first CRC match (pcc_enc.cpp:309-351). */
int dnrp_pcc_decode(const int16_t* llr, uint32_t plcf_type_test, uint8_t* plcf, uint32_t* closed_loop,
                    uint32_t* beamforming, uint32_t* iterations);

/* fec_t::encode_tb without the scrambling: tb [N_TB_bits/8] -> d [ceil(G/8)] (redundancy version
 * cfg->rv). DNRP_ECONFIG for a segmentation with filler bits (pdc_enc.cpp:144). */
int dnrp_pdc_encode(const dnrp_fec_cfg* cfg, const uint8_t* tb, uint8_t* d);
/* fec_t::decode_tb after the descrambling: the first n_llr <= G LLRs of the packet (code blocks
 * whose soft bits are not all present yet are left for a later call, pdc_enc.cpp:334-337) ->
 * tb [N_TB_bits/8]. Returns 1 if the transport block passed its CRC(s), 0 if not. hb: the HARQ
 * softbuffer to combine into (reset it for a new transport block), or NULL for a one-shot decode.
 * Up to 10 iterations per code block, CRC early stop after at least 2. */
int dnrp_pdc_decode(dnrp_harq_rx* hb, const dnrp_fec_cfg* cfg, const int16_t* llr, uint32_t n_llr, uint8_t* tb,
                    uint32_t* iterations);
/*
 * Device turbo decoding of m transport blocks <- fec_t::decode_tb for many packets at once (one-shot:
 * a fresh softbuffer, all G soft bits present), with the host decoder's arithmetic: each code block
 * decodes to the same bits after the same number of iterations as dnrp_pdc_decode.
 *   cfg         host [m]: N_TB_bits, N_bps, rv, G, Z of each packet
 *   llr         device, row i at llr + i*llr_stride (>= G_i): descrambled LLRs (dnrp_rx_pdc_batch output)
 *   tb          device, row i at tb + i*tb_stride (>= N_TB_bits_i/8 + 3): decoded transport block
 *               followed by its received CRC24A
 *   crc_ok      host [m]: 1 if every code block and the transport block passed their CRCs
 *   iterations  host [m] (optional): turbo iterations summed over the packet's code blocks
 * Blocking: returns after the work on the stream has completed.
 */
int dnrp_pdc_decode_batch(dnrp_ctx* ctx, uint32_t m, const dnrp_fec_cfg* cfg, const int16_t* llr, uint32_t llr_stride,
                          uint8_t* tb, uint32_t tb_stride, uint8_t* crc_ok, uint32_t* iterations, void* stream);
/* The same with HARQ soft combining (harq::buffer_rx_t on the device): per packet a softbuffer row
 * (softbuf + i*sb_stride int16, >= dnrp_pdc_softbuffer_size entries) and code-block CRC flags
 * (cb_crc + i*crc_stride, >= C bytes), both zeroed by the caller for a new transport block and kept
 * across its redundancy versions, like the host dnrp_pdc_decode with a dnrp_harq_rx: blocks that
 * passed earlier are neither combined nor decoded again (their bytes stay in the tb row, so pass the
 * same tb rows for every redundancy version), the others add the new soft bits; a transport-block
 * CRC failure after all block CRCs passed resets the packet's flags. Same results as the host path. */
int dnrp_pdc_decode_batch_harq(dnrp_ctx* ctx, uint32_t m, const dnrp_fec_cfg* cfg, const int16_t* llr,
                               uint32_t llr_stride, int16_t* softbuf, uint64_t sb_stride, uint8_t* cb_crc,
                               uint32_t crc_stride, uint8_t* tb, uint32_t tb_stride, uint8_t* crc_ok, uint32_t* iterations,
                               void* stream);
/* softbuffer entries (C * 3 * (K+ + 4)) and code blocks of a transport block (host only) */
int dnrp_pdc_softbuffer_size(uint32_t N_TB_bits, uint32_t Z, uint64_t* entries, uint32_t* n_cb);
/*
 * Device channel encoding of m transport blocks <- fec_t::encode_tb for many packets at once
 * (without the scrambling): bit-exact with dnrp_pdc_encode.
 *   tb  device, row i at tb + i*tb_stride (>= N_TB_bits_i/8)
 *   d   device, row i at d + i*d_stride (>= ceil(G_i/8)): the pdc_d rows dnrp_tx_batch takes
 * Blocking: returns after the work on the stream has completed.
 */
int dnrp_pdc_encode_batch(dnrp_ctx* ctx, uint32_t m, const dnrp_fec_cfg* cfg, const uint8_t* tb, uint32_t tb_stride,
                          uint8_t* d, uint32_t d_stride, void* stream);
/*
 * Device PLCF decoding of n PCCs <- fec_t::decode_plcf_test for many packets at once (after the
 * descrambling): turbo decoding (K = 56 / 96, up to 5 iterations, stop at the first CRC match) and
 * the CRC16 check under the four masks, with the host decoder's arithmetic (same bits, iterations).
 *   plcf_type_test  host [n]: 1 or 2 per packet
 *   llr             device, row i at llr + i*llr_stride (>= 196): dnrp_rx_pcc_batch's pcc_llr
 *   plcf            device, row i at plcf + i*plcf_stride (>= 10): the decoded PLCF (5 or 10 bytes)
 *   result          host [n]: 0 = no PLCF of that type; 1 + m for a CRC match under mask m
 *                   (0 none, 1 closed loop, 2 beamforming, 3 both: pcc_enc.cpp:170-183)
 *   iterations      host [n] (optional)
 * Blocking: returns after the work on the stream has completed.
 */
int dnrp_pcc_decode_batch(dnrp_ctx* ctx, uint32_t n, const uint32_t* plcf_type_test, const int16_t* llr,
                          uint32_t llr_stride, uint8_t* plcf, uint32_t plcf_stride, uint8_t* result, uint32_t* iterations,
                          void* stream);
/* Device PLCF encoding of n packets <- fec_t::encode_plcf for many packets at once (without the
 * scrambling): bit-exact with dnrp_pcc_encode.
 *   plcf_type host [n] (1 / 2); closed_loop, beamforming host [n] (optional, CRC mask selection)
 *   plcf      device, row i at plcf + i*plcf_stride (5 or 10 bytes)
 *   d         device, row i at d + i*d_stride (>= 25): dnrp_tx_batch's pcc_d rows
 * Blocking: returns after the work on the stream has completed. */
int dnrp_pcc_encode_batch(dnrp_ctx* ctx, uint32_t n, const uint32_t* plcf_type, const uint32_t* closed_loop,
                          const uint32_t* beamforming, const uint8_t* plcf, uint32_t plcf_stride, uint8_t* d,
                          uint32_t d_stride, void* stream);
int dnrp_harq_rx_create(uint32_t N_TB_bits_max, uint32_t Z, dnrp_harq_rx** out);
int dnrp_harq_rx_reset(dnrp_harq_rx* hb);
int dnrp_harq_rx_destroy(dnrp_harq_rx* hb);

const char* dnrp_strerror(int code);

#ifdef __cplusplus
}
#endif

#endif /* DNRP_H */
