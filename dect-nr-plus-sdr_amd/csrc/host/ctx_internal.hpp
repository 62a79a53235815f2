// Internal state of the C-ABI context shared by the host translation units (ctx.cpp: context and
// small tables, tables.cpp: per-configuration device tables, tx.cpp / rx.cpp: the TX and RX phase
// launches, sync.cpp: synchronisation). Not part of the public interface.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../kernels/kernels.hpp"
#include "dnrp.h"
#include "geometry.hpp"


#define HIPCHK(x)                                  \
    do {                                           \
        if ((x) != hipSuccess) return DNRP_EDEVICE; \
    } while (0)


namespace dnrp::host {

// device buffer owning wrapper
struct dbuf {
    void* p = nullptr;
    size_t n = 0;
    hipEvent_t busy = nullptr;  // per-call argument buffers: recorded after the last kernel reading it
    dbuf() = default;
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() {
        if (p) (void)hipFree(p);
        if (busy) (void)hipEventDestroy(busy);
    }
    // before refilling a per-call argument buffer on stream st: the kernels of an earlier call
    // (possibly on another stream) that read it must have finished
    hipError_t wait_idle(hipStream_t st) {
        if (!busy) return hipEventCreateWithFlags(&busy, hipEventDisableTiming);
        return hipStreamWaitEvent(st, busy, 0);
    }
    // after the launches reading it on stream st
    hipError_t mark_busy(hipStream_t st) {
        if (!busy && hipEventCreateWithFlags(&busy, hipEventDisableTiming) != hipSuccess) return hipErrorUnknown;
        return hipEventRecord(busy, st);
    }
    bool ensure(size_t bytes) {
        if (bytes <= n) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) return false;
        n = bytes;
        return true;
    }
    template <typename T>
    bool upload(const std::vector<T>& v) {
        if (!ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return false;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

struct pinned {
    void* p = nullptr;
    size_t n = 0;
    hipEvent_t ev = nullptr;
    ~pinned() {
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
    }
    void* get(size_t bytes) {
        if (!ev) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        (void)hipEventSynchronize(ev);  // previous async copy out of this buffer is done
        if (bytes > n) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            n = 0;
            if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
            n = bytes;
        }
        return p;
    }
};

dev::fft_plan make_plan(uint32_t N);
std::vector<float2> twiddles(uint32_t N);                   // forward, exp(-2 pi i j / N)
std::vector<float2> constellation(uint32_t N_bps);
std::vector<float> taps_polyphase(const geo::resampler_t& rs, uint32_t* count);
double phasor_arg(double rad);
void fill_pairs(uint32_t N_TS, uint32_t* pair, uint32_t& mod);
// the streaming TX kernel's code tables (tables.cpp; pure host code, dnrp_query_table "tx_code_oh")
bool tx_pair_codes(std::vector<uint32_t>& code, uint32_t N_TS);  // false: a cell index past the code word
std::vector<uint32_t> tx_code_bin(const std::vector<uint32_t>& code, uint32_t N_occ, uint32_t off_lower, uint32_t N_DF);
std::vector<uint32_t> tx_code_oh(const std::vector<uint32_t>& cb, const uint32_t* pdc_off, uint32_t N_DF, uint32_t N_TS, uint32_t N_SS,
                                 uint32_t N_bps, bool txdiv);

struct tx_tables {
    dnrp_packet_sizes q{};
    geo::tm_t tm{};
    geo::dims_t dm{};
    dev::fft_plan plan{};
    geo::resampler_t rs;
    dbuf code, stf, W, taps, taps_pp, tw, qam, qpsk, pdc_off;
    dbuf code_bin;  // [N_DF+1][1024] code per FFT bin, bin lane + 64 m at [m / 4][lane][m % 4] (streaming TX kernel, N_b_DFT_os = 1024)
    dbuf code_oh;   // [N_TS][N_DF+1][1024] one-hot W codes per antenna stream (kernels.hpp OH_*; empty: not built)
    uint32_t pcc_syms = 0;  // bit l: symbol l carries PCC cells
    uint32_t npp = 0;  // floats in taps_pp
    std::vector<float> wscale, wscale_opt;  // per codebook: standard / optimal_scaling_DAC
    std::vector<uint8_t> w_onehot;           // per codebook: one nonzero entry in every antenna row
    std::vector<uint32_t> pdc_off_h;  // host copy of maps.pdc_sym_off
};

// device copy of a geo::rx_plan_t
struct rx_plan_dev {
    uint32_t n_dops = 0, n_epochs = 0;
    bool cells_ok = true;  // every epoch fits rx_cells_kernel: <= CELL_MAX_SEGS segments, one DRS count
    dbuf dl, dmeta, segs, epochs;
    dbuf sym_op;  // [n_sym] first DRS op at symbol l, 0xFFFF: none (the front end's DRS test)
    uint32_t n_sym_op = 0;
    // residual STO tracking: the ops' symbols on the host and as a front-end symbol list (launch_fft_list)
    std::vector<uint32_t> dl_h;
    dbuf dl16;
    bool upload(const geo::rx_plan_t& p) {
        static_assert(sizeof(geo::rx_seg_t) == sizeof(dev::rx_seg), "rx_seg layout");
        static_assert(sizeof(geo::rx_epoch_t) == sizeof(dev::rx_epoch), "rx_epoch layout");
        n_dops = static_cast<uint32_t>(p.dl.size());
        n_epochs = static_cast<uint32_t>(p.epochs.size());
        for (const auto& e : p.epochs) {
            cells_ok = cells_ok && e.seg1 - e.seg0 <= dev::CELL_MAX_SEGS;
            for (uint32_t i = e.seg0; i < e.seg1; ++i) cells_ok = cells_ok && p.segs[i].drs_cnt == p.segs[e.seg0].drs_cnt;
        }
        uint32_t lmax = 0;
        for (uint32_t l : p.dl) lmax = std::max(lmax, l);
        std::vector<uint16_t> so((lmax + 2) & ~1u, 0xFFFFu);  // whole dwords (scalar loads)
        for (uint32_t d = n_dops; d-- > 0;) so[p.dl[d]] = static_cast<uint16_t>(d);
        n_sym_op = lmax + 1;
        dl_h = p.dl;
        const std::vector<uint16_t> l16(p.dl.begin(), p.dl.end());
        return dl.upload(p.dl) && dmeta.upload(p.dmeta) && segs.upload(p.segs) && epochs.upload(p.epochs) && sym_op.upload(so) &&
               dl16.upload(l16);
    }
};

struct rx1_tables {  // per (u, b, N_eff_TX): STF/PCC phase
    uint32_t u, b, N_eff_TX, Nd, N_occ, off_lower, CP, STF_CP, n_pattern, pattern_len;
    dev::fft_plan plan{};
    geo::resampler_t rs;
    geo::maps_t maps;
    uint32_t pcc_max = 0;
    bool drs_arith = false;  // DRS tables match rx_drs_partials' arithmetic (front-end SNR sums)
    dbuf stf, tw, taps, taps_pp, drs_k, drs_v, pcc_k, pcc_sym;
    uint32_t npp = 0;  // floats in taps_pp
    rx_plan_dev bplan;  // PCC phase back end
    dbuf lut_pw[2][3], lut_w[2][3], luts;
    dbuf lut_pair_w[2][3], lut_pair_p[2][3];  // SFBC pair union windows of full symbols (rx_lut::pair_w)
    uint32_t lut_n[2][3] = {}, lut_nw[2][3] = {}, lut_T[2] = {};
    uint32_t wcap[2] = {};  // largest weight table of mode l / lr (rx_cells_kernel LDS slots)
};

struct rx2_tables {  // per (psdef): PDC phase
    dnrp_packet_sizes q{};
    geo::maps_t maps;
    dbuf pdc_k, pdc_sym;
    rx_plan_dev bplan;  // PDC phase back end
    rx_plan_dev eplan;  // the same plan with twin segments, the epoch receiver's (eplan_ok; else it takes bplan)
    bool eplan_ok = false;
    bool sm = false;    // spatial multiplexing (N_SS > 1): MMSE cells kernel
    // MIMO report (estimator_mimo_t): wideband DRS cells, single-stream codebooks
    uint32_t N_TS = 1, ncb_tx = 0, A_tx = 0, ncb_rx = 0, A_rx = 0;
    dbuf mimo_cells, mimo_signs, Wtx, stx, Wrx, srx;
    // rx_mimo_detail_kernel (dnrp_ctx_set_rx_mimo_report): the spatial-multiplexing codebooks (R, N_TS) of the
    // rank slots R = 1, 2, 4 back to back in Wsm [entry][antenna][layer] / ssm (scaling factors): entries per
    // slot (0: rank not available at this N_TS), the slot's first float2 in Wsm and first entry in ssm
    uint32_t sm_ncb[3] = {}, sm_woff[3] = {}, sm_cboff[3] = {};
    dbuf Wsm, ssm;
    // fused PDC receiver (kernels/rx_fused.hip): its symbol table, the phase's DRS symbols the front
    // end runs first (after the PCC phase's), whether those carry PDC cells (their bins then go to Y),
    // and the MIMO report's wideband cells in the zero-forced pilots (op << 16 | DRS cell)
    bool fused_ok = false, drs_y = false;
    uint32_t n_fsym = 0, n_drs_syms = 0;
    dbuf fsym, drs_syms, mimo_zcells;
    // epoch receiver (kernels/rx_epoch.hip): per plan epoch the front-end symbols it owns (PDC-bearing,
    // after the PCC phase, not DRS: each in exactly one epoch), and the phase's DRS symbols for the
    // DRS pass ahead of it
    bool ep_ok = false;
    uint32_t n_ep_drs = 0;
    dbuf ep_off, ep_sym, ep_drs;
};

struct netid_seq {
    uint32_t nbits = 0;
    dbuf t1, t2;
};

// Run-time switches (environment variables): A/B and test hooks. Each is read at one fixed time, by the
// read_* function of that time below and nowhere else; tests flip the per-call ones on a live context.
struct switches {
    // ---- at context creation (read_create)
    bool timing = false;  // DNRP_TIMING=1 (first character '1'): HIP events around every launch
    bool eq_twin = true;  // DNRP_EQ_TWIN=0: no twin segments in the epoch receiver's plan (geo::build_rx_plan)
    // ---- once per PCC call, so that its PDC call agrees (read_pcc)
    bool rx_snr_front = true;  // DNRP_RX_SNR_FRONT=0: rx_snr gathers the DRS cells from Y (no front-end sums, no pilots)
    // DNRP_RX_FUSED=1 (and rx_snr_front): the PDC phase through the fused receiver (rx_fused.hip) instead
    // of Y and rx_cells: parity-tested, slower on MI355X (docs/DESIGN_LOG.md §6)
    bool rx_fused = false;
    // DNRP_RX_EPOCH: the PDC phase through the epoch receiver (rx_epoch.hip) -- 1 (default) with 4 or more RX
    // antennas, where it measured faster (C4: 1.2 ms per 16384-slot chunk; SISO C3 loses, 7.2 vs 5.5 ms per
    // 8192: one symbol task per wave and epoch), 2 for every geometry it supports, 0 never (Y + rx_cells)
    uint32_t rx_epoch = 1;
    uint32_t rx_group = 0;  // DNRP_RX_GROUP=G: the Y path in groups of G packets on two streams (0: one launch set)
    // ---- per TX call (read_tx)
    uint64_t tx_big_cap = uint64_t(4) << 30;  // DNRP_TX_BIG_CAP (bytes) lowers it: a test can force several passes
    // DNRP_TX_MFMA=1 / 2 (f32): polyphase blocks on the matrix cores (polyphase.hpp mf_blocks), opt-in A/B;
    // the VALU blocks measured faster (docs/DESIGN_LOG.md)
    uint32_t tx_mfma = 0;
    // ---- per sync call (read_sync)
    // DNRP_SYNC_ROUNDS: split detection / coarse-peak rounds ahead of the inline detection. -1 (unset): 2
    // with several antennas (their peak searches in parallel instead of in series: C4 4 antennas 199k -> 205k
    // slot-pairs/s), 0 with one (the extra dependent launches lengthen the chain the host waits on: C3 654k
    // inline vs 573k split, C2 equal; same-box A/B on MI355X)
    int sync_rounds = -1;
    // DNRP_SYNC_STREAM=0: the wave step-sum kernel; DNRP_SYNC_PIPE=0: the streaming one with the single-chunk
    // prefetch; default the pipelined one (one wave per workgroup, a retired segment frees its LDS at once:
    // sync_steps 4.32 -> 3.81 ms, 176.4k -> 186.0k slot-pairs/s against four waves)
    dev::sync_steps_kind sync_steps = dev::SYNC_STEPS_PIPE;
    // DNRP_SYNC_TRANCHE: 0 = one tranche; "32,64" = explicit tranche sizes in steps (geo::sync_tranches' forced)
    bool sync_tranche_set = false;
    std::vector<uint64_t> sync_tranche;
};

inline void read_create(switches& s) {
    const char *tm = std::getenv("DNRP_TIMING"), *tw = std::getenv("DNRP_EQ_TWIN");
    s.timing = tm && tm[0] == '1';
    s.eq_twin = !tw || std::atoi(tw) != 0;
}
inline void read_pcc(switches& s) {
    const char *e = std::getenv("DNRP_RX_SNR_FRONT"), *f = std::getenv("DNRP_RX_FUSED");
    const char *ep = std::getenv("DNRP_RX_EPOCH"), *gr = std::getenv("DNRP_RX_GROUP");
    s.rx_snr_front = !e || std::atoi(e);
    s.rx_fused = s.rx_snr_front && f && std::atoi(f);
    s.rx_epoch = ep ? static_cast<uint32_t>(std::atoi(ep)) : 1u;
    s.rx_group = gr ? static_cast<uint32_t>(std::atoi(gr)) : 0u;
}
inline void read_tx(switches& s) {
    const char *e = std::getenv("DNRP_TX_BIG_CAP"), *mf = std::getenv("DNRP_TX_MFMA");
    s.tx_big_cap = std::min<uint64_t>(uint64_t(4) << 30, e ? std::strtoull(e, nullptr, 10) : ~uint64_t(0));
    s.tx_mfma = mf ? static_cast<uint32_t>(std::min(2, std::max(0, std::atoi(mf)))) : 0u;
}
inline void read_sync(switches& s) {
    const char *rd = std::getenv("DNRP_SYNC_ROUNDS"), *ss = std::getenv("DNRP_SYNC_STREAM");
    const char *pp = std::getenv("DNRP_SYNC_PIPE"), *tr = std::getenv("DNRP_SYNC_TRANCHE");
    s.sync_rounds = rd ? std::max(0, std::atoi(rd)) : -1;
    s.sync_steps = ss && !std::atoi(ss) ? dev::SYNC_STEPS_WAVE : pp && !std::atoi(pp) ? dev::SYNC_STEPS_STREAM : dev::SYNC_STEPS_PIPE;
    s.sync_tranche_set = tr != nullptr;
    s.sync_tranche.clear();
    for (char* q = nullptr; tr && *tr; tr = q + 1) {
        const unsigned long v = std::strtoul(tr, &q, 10);
        if (q == tr) break;
        s.sync_tranche.push_back(v);
        if (*q != ',') break;
    }
}

struct sync_tables {  // per (u, b) of the searched STF: sync_chunk_t / crosscorrelator_t constructors
    uint32_t u = 0, b = 0, n_pattern = 0, stf_len = 0, pattern = 0, step = 0, D = 0, bos = 0;
    uint32_t xc_l = 0, xc_len = 0, tmpl_len = 0, n_templates = 0, log2_fft = 0;
    float rms_min = 0.f;
    geo::resampler_t rs;  // sync resampler (RX direction)
    uint32_t m_star = 0, p_star = 0, npp = 0;
    dbuf taps, taps_pp, tmpl_f, tw_fft;
    // beta search (dnrp_ctx_set_sync_beta_search), built at its first use for this (u, b): template
    // spectra [b_idx][n_templates][n_fft] of every b <= this b, plan and twiddles of the 64 bos-point transform
    // (plan and twiddles: coarse_fft_ready, shared with the integer CFO search)
    bool beta_ready = false, coarse_fft_ready = false;
    dbuf tmpl_fb, tw_beta;
    dev::fft_plan beta_plan{};
};

// rx.cpp: the azimuth grid of an angle-of-arrival setting and its steering table, for the device scan
// (dnrp_ctx_set_rx_aoa uploads it) and the host twin (dnrp_aoa_estimate) alike
struct aoa_grid {
    uint32_t n_grid = 0, cyclic = 0;
    double az0 = 0.0, step = 0.0;  // az_g = az0 + g step
};
bool aoa_cfg_ok(const dnrp_aoa_cfg* cfg);
aoa_grid aoa_grid_of(const dnrp_aoa_cfg& cfg);
std::vector<double2> aoa_steering(const dnrp_aoa_cfg& cfg, const aoa_grid& g, uint32_t N_RX);  // [n_grid][N_RX]

// tables.cpp: the tables of a configuration, built and uploaded at its first use (nullptr: *err set)
tx_tables* get_tx(dnrp_ctx* ctx, const dnrp_psdef& d, int* err);
rx1_tables* get_rx1(dnrp_ctx* ctx, uint32_t u, uint32_t b, uint32_t N_eff_TX, int* err);
rx2_tables* get_rx2(dnrp_ctx* ctx, const dnrp_psdef& d, int* err);
// ctx.cpp: the PDC scrambling sequences of a network ID, at least nbits long
int ensure_seq(dnrp_ctx* ctx, netid_seq& s, uint32_t nid, uint32_t nbits);
// rx.cpp: front-end arguments of a PCC-phase geometry; plan: the phase plan whose DRS SNR sums (and
// pilots) the front end computes, where it does
dev::rx_front_args front_args(dnrp_ctx* ctx, rx1_tables* t, const float* iq, const uint32_t* sel,
                              const rx_plan_dev* plan = nullptr);

}  // namespace dnrp::host

struct dnrp_ctx {
    using tx_tables = dnrp::host::tx_tables;
    using rx1_tables = dnrp::host::rx1_tables;
    using rx2_tables = dnrp::host::rx2_tables;
    using netid_seq = dnrp::host::netid_seq;
    using dbuf = dnrp::host::dbuf;
    using pinned = dnrp::host::pinned;
    dnrp_cfg cfg{};
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, std::unique_ptr<tx_tables>> txt;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::unique_ptr<rx1_tables>> rx1t;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, std::unique_ptr<rx2_tables>> rx2t;
    std::map<uint32_t, std::unique_ptr<netid_seq>> netid;
    dbuf pcc_seq;
    // batch scratch
    dbuf tx_pk, rx_in, rx_st, Y, pdc_seq_ptrs, lut_d, nv_d, mimo_out;
    dbuf tx_big;  // N_b_DFT_os > 1024: DECT-rate symbols [n][N_TX][big_len] (tx.hip tx_big_sym_kernel)
    // TX OFDM windowing (dnrp_ctx_set_tx_windowing): the fraction of later TX calls (0: off) and the
    // rising edges uploaded so far, one per (N_b_DFT_os, fraction bits)
    float tx_win_fraction = 0.0f;
    dnrp::dev::tx_form tx_form{};  // kernel form of the latest dnrp_tx_batch that launched (dnrp_tx_last_form)
    bool tx_form_valid = false;
    std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<dbuf>> tx_win;
    dbuf stf_part;  // [max_batch][8] double2 cs | [max_batch][8] float rms | [max_batch][8][14 b_max] float2 cells
    dbuf snr_part;  // [slot][n_sym_total][N_RX][8] double2: front-end DRS SNR partial sums
    // zero-forced DRS pilots [slot][zd_dops][N_RX][4][zd_row] (rx_front_args::zd); op zd_dops - 1 of
    // every slot stays zero (the fused receiver's op-less interlace slots), zd_key: layout it was zeroed for
    dbuf zd;
    uint32_t zd_dops = 0, zd_row = 0;
    std::tuple<void*, size_t, uint32_t, uint32_t, uint32_t> zd_key{};
    dnrp::host::switches sw;  // each section as of its read time
    // PDC phase in packet groups (sw.rx_group): the back ends' stream, fork / join through rx_fork / rx_join
    hipStream_t rx_aux = nullptr;
    hipEvent_t rx_fork = nullptr, rx_join = nullptr;
    uint32_t rx_mode = 0;  // DNRP_RX_MODE_* (dnrp_ctx_set_rx_mode)
    // residual STO tracking from the DRS symbols (dnrp_ctx_set_rx_sto_tracking): the setting, and what the
    // latest dnrp_rx_pcc_batch read of it (rx_sto_on / rx_sto_gain hold for that call's PDC call);
    // sto_sym: [slot][rx_nsym_cap + 1] increment each symbol was derotated with, NaN where none was
    uint32_t sto_track_on = 0;
    float sto_track_gain = 1.0f;
    bool rx_sto_on = false;
    float rx_sto_gain = 1.0f;
    dbuf sto_sym;
    // residual CFO tracking (dnrp_ctx_set_rx_cfo_tracking) likewise; cfo_sym: [slot][rx_nsym_cap + 1] mixer entry
    // (phase a, increment) each symbol was mixed with; cfo_keep: the PCC phase's zero-forced DRS pilots
    // [slot][RX_CFO_KEEP][N_RX][4][14 b_max], which the PDC phase's first pairs reach back to
    uint32_t cfo_track_on = 0;
    float cfo_track_gain = 1.0f;
    bool rx_cfo_on = false;
    float rx_cfo_gain = 1.0f;
    dbuf cfo_sym, cfo_keep;
    // MIMO report options (dnrp_ctx_set_rx_mimo_report): the setting, read once per dnrp_rx_pdc_batch.
    // mimo_rows: one dnrp_mimo_detail per request of the latest PDC call that ran rx_mimo_detail_kernel, sized
    // like mimo_out; mimo_rows_m: that call's m where it ran with detail = 1, else 0 (dnrp_rx_mimo_detail)
    uint32_t mimo_metric = 0, mimo_all_w = 0, mimo_detail = 0;
    uint32_t mimo_rows_m = 0;
    dbuf mimo_rows;
    // angle-of-arrival report (dnrp_ctx_set_rx_aoa): the setting with its steering table, null = off; every setter
    // call makes a new object, so the launches of a PDC call in flight keep the table they took (aoa_used: the
    // latest PDC call's, alive until the next one replaces it). aoa_rows: one dnrp_aoa_report per request of the
    // latest PDC call that ran rx_aoa_kernel, aoa_rows_m: that call's m, else 0 (dnrp_rx_aoa)
    struct aoa_setting {
        dnrp_aoa_cfg cfg{};
        dnrp::host::aoa_grid grid{};
        dbuf steer;  // [n_grid][N_RX] double2
    };
    std::shared_ptr<aoa_setting> aoa, aoa_used;
    uint32_t aoa_rows_m = 0;
    dbuf aoa_rows;
    pinned st_tx, st_rxin, st_seq, st_rep;
    // retained RX phase-1 state: per PCC-batch slot its (u, b, N_eff_TX) tables and symbol
    // capacity; Y is laid out with the batch-wide maxima rx_nsym_cap / rx_Nf_pad
    bool rx_valid = false;
    uint32_t rx_n = 0, rx_S_in = 0, rx_nsym_cap = 0, rx_Nf_pad = 0, rx_n_windows = 0;
    const float* rx_iq = nullptr;  // the PCC call's windows: the PDC call must read the same ones
    std::vector<rx1_tables*> rx_slot_t;
    std::vector<uint32_t> rx_slot_cap;
    dbuf rx_sel, rx_sel2;  // [max_batch][2] launch packet -> slot / output row (PCC / PDC call), one slice per group
    pinned st_sel, st_sel2;
    // synchronisation: per (u, b) tables, step sums and reports
    std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<dnrp::host::sync_tables>> synct;
    dbuf sy_P, sy_C, sy_res, sy_cnt, sy_spec, sy_post, sy_state, sy_pk;
    // beta search at the coarse peak (dnrp_ctx_set_sync_beta_search): off, or the sideband threshold of
    // later sync calls in dB; sy_band: [n * max_reports][8][6] band powers per antenna (sync_beta_kernel)
    uint32_t sync_beta_on = 0;
    float sync_beta_db = -10.0f;
    dbuf sy_band;
    // fine search over every antenna with a coarse peak (dnrp_ctx_set_sync_fine_all_antennas): the setting
    // of later sync calls; sy_fine_m / sy_fine_i: the per-antenna table [n * max_reports][8][4] of the latest
    // dnrp_rx_sync_batch that ran with it on, sync_fine_reports its n * max_reports (0: none, or it ran off)
    uint32_t sync_fine_all = 0;
    uint32_t sync_fine_reports = 0;
    dbuf sy_fine_m, sy_fine_i;
    // integer CFO search at the coarse peak (dnrp_ctx_set_sync_icfo_search): 0 = off, or the candidate range of
    // later sync calls; sy_icfo: the score table [n * max_reports][8][9] of the latest dnrp_rx_sync_batch that ran
    // with it on, sync_icfo_reports its n * max_reports (0: none, or it ran off), sync_icfo_ant its antennas
    uint32_t sync_icfo_range = 0;
    uint32_t sync_icfo_reports = 0, sync_icfo_ant = 0;
    dbuf sy_icfo;
    // ring-buffer gather / continuous-stream synchronisation (stream.cpp)
    dbuf ring_start, ring_win;
    pinned st_ring, st_stream;
    // simulated channel (channel.cpp): per-call link realisations
    dbuf chan_tab;
    pinned st_chan;
    // virtual space (vspace.cpp): per-call emissions, tile plan and link realisations
    dbuf vs_tab;
    pinned st_vs;
    // channel scanner (stream.cpp): per-call partial scans, their RMS values
    dbuf chscan_tab, chscan_rms;
    pinned st_chscan, st_chscan_out;
    // timing: HIP events recorded on the caller's stream around every launch (sw.timing)
    struct ev_pool {
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
        size_t used = 0;
    };
    std::map<std::string, ev_pool> ev;
    // device turbo decoding (fec.cpp dnrp_pdc_decode_batch, kernels/fec.hip): per-size tables
    // (circular-buffer lists) built at the first call, plan and work buffers
    dbuf fec_tab, fec_cbs, fec_waves, fec_work16, fec_tail, fec_bits, fec_ck, fec_cbout, fec_tbarg;
    dbuf fec_cbs2, fec_waves2, fec_map2, fec_work16b, fec_tailb, fec_cbout2;  // continuation of undecided blocks
    std::vector<uint32_t> fec_valid_off, fec_start;  // per K index ([idx][rv] for start)
    ~dnrp_ctx() {
        if (rx_aux) (void)hipStreamDestroy(rx_aux);
        if (rx_fork) (void)hipEventDestroy(rx_fork);
        if (rx_join) (void)hipEventDestroy(rx_join);
        for (auto& e : ev)
            for (auto& p : e.second.ev) {
                (void)hipEventDestroy(p.first);
                (void)hipEventDestroy(p.second);
            }
    }
    void tic(const char* name, hipStream_t s) {
        if (!sw.timing) return;
        auto& pool = ev[name];
        if (pool.used == pool.ev.size()) {
            std::pair<hipEvent_t, hipEvent_t> p{};
            (void)hipEventCreate(&p.first);
            (void)hipEventCreate(&p.second);
            pool.ev.push_back(p);
        }
        (void)hipEventRecord(pool.ev[pool.used].first, s);
    }
    void toc(const char* name, hipStream_t s) {
        if (!sw.timing) return;
        auto& pool = ev[name];
        (void)hipEventRecord(pool.ev[pool.used].second, s);
        ++pool.used;
    }
};
