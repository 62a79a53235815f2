// dnrp_rx_pcc_batch / dnrp_rx_pdc_batch (include/dnrp.h): the launches of the two RX phases.
#include <cstddef>

#include "ctx_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace {

// the DRS SNR sums of a phase come from the front end (rx_fft_wave_kernel) where it runs; both phases
// of a packet use the same PCC-phase geometry t, so the PCC and PDC launches agree
bool snr_from_front(dnrp_ctx* ctx, rx1_tables* t) {
    return ctx->sw.rx_snr_front && t->drs_arith && dev::rx_fft_wave_path(front_args(ctx, t, nullptr, nullptr));
}

// one phase (PCC or PDC) of a launch group: what its back end works on
struct rx_phase {
    rx1_tables* t;            // PCC-phase geometry of the group
    const rx_plan_dev* plan;  // the phase's plan
    uint32_t n;               // launch packets
    const uint32_t* sel;      // launch packet -> slot / output row
    bool pdc;
    uint32_t N_bps;
    const uint32_t* kk;  // the phase's cells: subcarrier index, OFDM symbol
    const uint16_t* cell_sym;
    int16_t* llr;
    uint32_t llr_stride;
    bool sm;  // spatial multiplexing: the MMSE cells kernel
};

// the phase's DRS ops as the SNR chain, the trackers and the cells kernels see them
dev::rx_drs_view drs_view(dnrp_ctx* ctx, const rx_phase& p) {
    dev::rx_drs_view v{};
    v.N_RX = ctx->cfg.N_TX_max;
    v.Nf_pad = ctx->rx_Nf_pad;
    v.n_sym_total = ctx->rx_nsym_cap + 1;
    v.n_drs = p.t->N_occ / 4;
    v.n_dops = p.plan->n_dops;
    v.is_pdc = p.pdc;
    v.dl = p.plan->dl.as<uint32_t>();
    v.dmeta = p.plan->dmeta.as<uint32_t>();
    v.drs_k = p.t->drs_k.as<uint32_t>();
    v.drs_v = p.t->drs_v.as<float>();
    v.Y = ctx->Y.as<float2>();
    v.st = ctx->rx_st.as<dev::rx_pkt_state>();
    v.sel = p.sel;
    return v;
}

// the cells kernels' arguments of one phase (rx_cells_kernel, rx_epoch_kernel). lut_d and nv_d are
// sized by dnrp_rx_pcc_batch, so their addresses hold whenever a block is built
dev::rx_cells_args cells_args(dnrp_ctx* ctx, const rx_phase& p) {
    const rx1_tables* t = p.t;
    const dev::rx_drs_view v = drs_view(ctx, p);
    dev::rx_cells_args c{};
    c.N_occ = t->N_occ;
    c.N_RX = v.N_RX;
    c.NT = t->N_eff_TX;
    c.Nf_pad = v.Nf_pad;
    c.n_sym_total = v.n_sym_total;
    c.n_drs = v.n_drs;
    c.n_dops = v.n_dops;
    c.n_epochs = p.plan->n_epochs;
    c.n_pkt = p.n;
    c.N_bps = p.N_bps;
    c.wcap[0] = t->wcap[0];
    c.wcap[1] = t->wcap[1];
    fill_pairs(t->N_eff_TX, c.pair, c.mod);
    c.is_pdc = v.is_pdc;
    c.sm = p.sm ? 1u : 0u;
    c.nv_d = ctx->nv_d.as<float>();
    c.epochs = p.plan->epochs.as<dev::rx_epoch>();
    c.segs = p.plan->segs.as<dev::rx_seg>();
    c.dl = v.dl;
    c.dmeta = v.dmeta;
    c.drs_k = v.drs_k;
    c.drs_v = v.drs_v;
    c.kk = p.kk;
    c.cell_sym = p.cell_sym;
    c.luts = t->luts.as<dev::rx_lut>();
    c.Y = v.Y;
    c.lut_d = ctx->lut_d.as<uint8_t>();
    c.pcc_seq = ctx->pcc_seq.as<uint8_t>();
    c.pdc_seq = static_cast<const uint8_t* const*>(ctx->pdc_seq_ptrs.p);
    c.llr = p.llr;
    c.llr_stride = p.llr_stride;
    c.sel = v.sel;
    return c;
}

// back-end launches of one phase: the SNR chain (rx_drs.hip), then the cells kernel on c (rx_cells.hip); c
// null: the SNR chain only (launch_snr_chain)
int launch_back(dnrp_ctx* ctx, const rx_phase& p, const dev::rx_cells_args* c, hipStream_t st) {
    rx1_tables* t = p.t;
    const rx_plan_dev& plan = *p.plan;
    const char* name = p.pdc ? "rx_pdc" : "rx_pcc";
    if (plan.n_dops > dev::RX_MAX_DOPS || (c && !plan.cells_ok)) return DNRP_EUNSUPPORTED;
    if (c) {  // the cells kernels' LDS staging (rx_cells.hip): a geometry beyond one CU is unsupported
        const uint32_t R = ctx->cfg.N_TX_max, T = t->N_eff_TX;
        if (dev::cell_lds_bytes(R, T, t->N_occ / 4, t->wcap[0], t->wcap[1]) > dev::LDS_BYTES) return DNRP_EUNSUPPORTED;
        // the MMSE cells kernel's instantiations
        if (p.sm && !dev::rx_cells_supported(R, T, true)) return DNRP_EUNSUPPORTED;
    }
    dev::rx_snr_args s{};
    s.V = drs_view(ctx, p);
    for (int i = 0; i < 3; ++i) s.prof_snr[i] = geo::lut_profile_snr_db(i);
    s.lut_d = ctx->lut_d.as<uint8_t>();
    s.nv_d = ctx->nv_d.as<float>();
    s.snr_part = snr_from_front(ctx, t) ? ctx->snr_part.as<double2>() : nullptr;
    ctx->tic(name, st);
    if (dev::launch_rx_snr(s, p.n, st) != hipSuccess) return DNRP_EDEVICE;
    if (c && plan.n_epochs &&
        (p.sm ? dev::launch_rx_cells_sm(*c, p.n, st) : dev::launch_rx_cells(*c, p.n, st)) != hipSuccess)
        return DNRP_EDEVICE;
    ctx->toc(name, st);
    return DNRP_OK;
}

// the fused and the epoch receiver equalise themselves: they take the LUT picks of the SNR chain alone
int launch_snr_chain(dnrp_ctx* ctx, const rx_phase& p, hipStream_t st) { return launch_back(ctx, p, nullptr, st); }

}  // namespace

dev::rx_front_args dnrp::host::front_args(dnrp_ctx* ctx, rx1_tables* t, const float* iq, const uint32_t* sel,
                                          const rx_plan_dev* plan) {
    dev::rx_front_args a{};
    a.plan = t->plan;
    a.N_occ = t->N_occ;
    a.off_lower = t->off_lower;
    a.CP = t->CP;
    a.STF_CP = t->STF_CP;
    a.N_RX = ctx->cfg.N_TX_max;
    a.S_in = ctx->rx_S_in;
    a.n_pattern = t->n_pattern;
    a.pattern_len = t->pattern_len;
    a.b = t->b;
    a.L = t->rs.L;
    a.M = t->rs.M;
    a.delay = t->rs.delay;
    a.hl = t->rs.hl;
    const auto al = geo::resampler_align(t->rs);
    a.m_star = al.m_star;
    a.p_star = al.p_star;
    a.sym_per_block = 4;
    a.Nf_pad = ctx->rx_Nf_pad;
    a.n_sym_total = ctx->rx_nsym_cap + 1;
    a.amp_scale = std::sqrt(static_cast<float>(t->N_occ)) / static_cast<float>(t->Nd);
    a.taps = t->taps.as<float>();
    a.taps_pp = t->taps_pp.as<float>();
    a.npp = t->npp;
    a.tw = t->tw.as<float2>();
    a.stf = t->stf.as<float2>();
    a.iq = reinterpret_cast<const float2*>(iq);
    a.sel = sel;
    a.pin = ctx->rx_in.as<dev::rx_pkt_in>();
    a.st = ctx->rx_st.as<dev::rx_pkt_state>();
    a.Y = ctx->Y.as<float2>();
    {  // STF per (packet, antenna) scratch (dnrp_rx_pcc_batch sizes it): cs | rms | cells
        const size_t mb = ctx->cfg.max_batch;
        a.stf_cs = ctx->stf_part.as<double2>();
        a.stf_rms = reinterpret_cast<float*>(a.stf_cs + mb * 8);
        a.stf_ys = reinterpret_cast<float2*>(a.stf_rms + mb * 8);
        a.stf_ys_stride = 14 * ctx->cfg.b_max;
    }
    // compile-time-tap front end (rx.hip rx_fft_wave_kernel<.., true>) where the run-time taps are
    // the generated ones bit for bit (the tap-table variant measured slower, docs/DESIGN_LOG.md §6)
    a.stream = dev::rx_stream_taps_match(t->rs.h.data(), t->rs.h.size()) ? 1u : 0u;
    if (plan && dev::rx_fft_wave_path(a)) {
        a.snr_part = ctx->snr_part.as<double2>();
        a.dl = plan->dl.as<uint32_t>();
        a.dmeta = plan->dmeta.as<uint32_t>();
        a.n_dops = plan->n_dops;
        a.n_drs = t->N_occ / 4;
        a.drs_neg = geo::drs_neg_mask();
        a.sym_op = plan->sym_op.as<uint16_t>();
        a.n_sym_op = plan->n_sym_op;
        // the zero-forced pilots next to the SNR sums (the fused PDC receiver's source), where the
        // plan's ops fit below the zero op
        if (ctx->sw.rx_fused && ctx->zd.p && plan->n_dops + 1 <= ctx->zd_dops) {
            a.zd = ctx->zd.as<float2>();
            a.zd_dops = ctx->zd_dops;
            a.zd_row = ctx->zd_row;
        }
    }
    a.n_drs = t->N_occ / 4;
    return a;
}

namespace {

// ---- the PDC phase of one launch group: four receivers, one choice
enum class pdc_path {
    fused,      // rx_fused.hip: front end and equaliser per (packet, symbol), pilots from zd, no Y round trip
    epoch,      // rx_epoch.hip: front end and equaliser per (packet, epoch)
    grouped_y,  // Y + rx_cells in packet groups on two streams (sw.rx_group)
    plain_y,    // Y + rx_cells, one launch set
};

// every eligibility condition of the receivers, in order of preference. fa: the group's front-end
// arguments (with the pilots zd where the front end writes them), ca: its cells arguments
// sto_track: residual STO or CFO tracking is on (dnrp_ctx_set_rx_sto_tracking, dnrp_ctx_set_rx_cfo_tracking);
// the fused receiver and the grouped Y path, the two measured-slower alternatives, do not take the per-symbol
// tables and are never chosen then
// aoa: the angle-of-arrival report is on (dnrp_ctx_set_rx_aoa); it reads the packet's DRS rows from Y, where the
// fused receiver does not leave them
pdc_path choose_pdc_path(const switches& sw, const rx1_tables* t, const rx2_tables* t2, const dev::rx_front_args& fa,
                         const dev::rx_cells_args& ca, uint32_t ng, bool sto_track, bool aoa) {
    // both fused forms: the compile-time-tap wave front end and an instantiated (N_RX, N_eff_TX) pair
    const bool wave = fa.stream && dev::rx_fft_wave_path(fa);
    if (!sto_track && !aoa && sw.rx_fused && t2->fused_ok && fa.zd && wave && dev::rx_fused_supported(fa.N_RX, t->N_eff_TX) &&
        dev::rx_fused_lds(fa.N_RX) <= dev::LDS_BYTES)
        return pdc_path::fused;
    if ((sw.rx_epoch >= 2 || (sw.rx_epoch == 1 && fa.N_RX >= 4)) && t2->ep_ok && !t2->sm && wave &&
        t2->bplan.cells_ok && t2->bplan.n_epochs && dev::rx_epoch_supported(fa.N_RX, t->N_eff_TX) &&
        dev::rx_epoch_lds(ca) <= dev::LDS_BYTES)
        return pdc_path::epoch;
    if (!sto_track && sw.rx_group && ng > sw.rx_group && t2->q.N_DF_symb > t->pcc_max) return pdc_path::grouped_y;
    return pdc_path::plain_y;
}

bool rx_tracking(const dnrp_ctx* ctx) { return ctx->rx_sto_on || ctx->rx_cfo_on; }  // what the PCC call read

// front end over a symbol list (the phase's DRS symbols) ahead of a fused receiver, or ahead of
// rx_sto_track_kernel. The wave front ends take the device list; rx_fft_kernel works on runs of
// consecutive symbols, so it takes the host copy syms_h, one launch per symbol
int launch_fft_list(dnrp_ctx* ctx, dev::rx_front_args fa, const uint16_t* syms, uint32_t count, uint32_t n, hipStream_t st,
                    const uint32_t* syms_h = nullptr) {
    if (!count) return DNRP_OK;
    const bool wave = dev::rx_fft_wave_path(fa);
    if (!wave && !syms_h) return DNRP_EUNSUPPORTED;
    ctx->tic("rx_fft_pdc", st);
    for (uint32_t i = 0; i < (wave ? 1u : count); ++i) {
        fa.sym_first = wave ? 0u : syms_h[i];
        fa.sym_list = wave ? syms : nullptr;
        fa.sym_count = wave ? count : 1u;
        if (dev::launch_rx_fft(fa, n, st) != hipSuccess) return DNRP_EDEVICE;
    }
    ctx->toc("rx_fft_pdc", st);
    return DNRP_OK;
}

// the trackers that are on, over one phase's symbols [sym_first, sym_last], on the Y rows a DRS pass with the STF
// values left (one pass for both: each measures the same rows; rx_sto_track_kernel, then rx_cfo_track_kernel);
// fa then carries their tables for the phase's launches
int launch_track(dnrp_ctx* ctx, const rx_phase& p, uint32_t sym_first, uint32_t sym_last, dev::rx_front_args& fa,
                 hipStream_t st) {
    const rx1_tables* t = p.t;
    auto common = [&](dev::rx_track_args& a, double gain) {
        a.V = drs_view(ctx, p);
        a.sym_first = sym_first;
        a.sym_last = sym_last;
        a.gain = gain;
    };
    if (ctx->rx_sto_on) {
        dev::rx_sto_args a{};
        common(a, ctx->rx_sto_gain);
        a.N_occ = t->N_occ;
        a.tab = ctx->sto_sym.as<double>();
        ctx->tic("rx_sto_track", st);
        if (dev::launch_rx_sto_track(a, p.n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("rx_sto_track", st);
        fa.sto_sym = a.tab;
    }
    if (ctx->rx_cfo_on) {
        if (t->bplan.n_dops > dev::RX_CFO_KEEP) return DNRP_EUNSUPPORTED;  // the PCC phase's pilots kept for the PDC phase
        dev::rx_cfo_args a{};
        common(a, ctx->rx_cfo_gain);
        a.n_stf = t->STF_CP + t->Nd;
        a.sym_len = t->CP + t->Nd;
        a.Nd = t->Nd;
        a.pin = ctx->rx_in.as<dev::rx_pkt_in>();
        a.tab = ctx->cfo_sym.as<double2>();
        a.keep = ctx->cfo_keep.as<float2>();
        ctx->tic("rx_cfo_track", st);
        if (dev::launch_rx_cfo_track(a, p.n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("rx_cfo_track", st);
        fa.cfo_sym = a.tab;
    }
    return DNRP_OK;
}

// A phase's front-end launches `pass(fa)` under residual STO / CFO tracking: first `pre(fa)`, launches that leave
// the phase's DRS rows in Y with the STF values, then the trackers on those rows, then `pass` with their tables
// in fa. Without tracking: `pass` alone.
template <class Pre, class Pass>
int tracked_pass(dnrp_ctx* ctx, const rx_phase& p, uint32_t sym_first, uint32_t sym_last, dev::rx_front_args& fa,
                 hipStream_t st, Pre&& pre, Pass&& pass) {
    if (rx_tracking(ctx)) {
        int err = pre(fa);
        if (err == DNRP_OK) err = launch_track(ctx, p, sym_first, sym_last, fa, st);
        if (err != DNRP_OK) return err;
    }
    return pass(fa);
}

// the phase's DRS symbols first (pilots, SNR sums; their bins to Y only where they carry PDC cells),
// then the SNR chain / LUT picks, then one fused launch for every PDC symbol
int pdc_fused(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, dev::rx_front_args fa, hipStream_t st) {
    fa.no_y = t2->drs_y ? 0u : 1u;
    int err = launch_fft_list(ctx, fa, t2->drs_syms.as<uint16_t>(), t2->n_drs_syms, p.n, st);
    if (err == DNRP_OK) err = launch_snr_chain(ctx, p, st);
    if (err != DNRP_OK) return err;
    dev::rx_fused_args x{};
    x.F = fa;
    x.n_pkt = p.n;
    x.n_fsym = t2->n_fsym;
    x.NT = p.t->N_eff_TX;
    x.N_bps = p.N_bps;
    uint32_t pr[12];
    fill_pairs(p.t->N_eff_TX, pr, x.mod);
    for (uint32_t i = 0; i < x.mod && i < 8; ++i) x.pair_bits |= uint64_t(pr[i] & 0xFFu) << (8 * i);
    x.fsym = t2->fsym.as<dev::rx_fsym>();
    x.kk = p.kk;
    x.luts = p.t->luts.as<dev::rx_lut>();
    x.lut_d = ctx->lut_d.as<uint8_t>();
    x.pdc_seq = static_cast<const uint8_t* const*>(ctx->pdc_seq_ptrs.p);
    x.llr = p.llr;
    x.llr_stride = p.llr_stride;
    ctx->tic("rx_fused", st);
    if (dev::launch_rx_fused(x, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("rx_fused", st);
    return DNRP_OK;
}

// DRS pass (the phase's DRS symbols: pilots in Y, SNR sums), the SNR chain's LUT picks, then one
// workgroup per (packet, epoch): front end of the epoch's symbols + equaliser, on the twin plan where
// the phase has one. With residual STO / CFO tracking the DRS pass feeds the tracking kernels and is repeated
// with their tables, which the epoch kernel's front end takes too
int pdc_epoch(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, dev::rx_front_args fa,
              const dev::rx_cells_args& ca, hipStream_t st) {
    auto drs_pass = [&](const dev::rx_front_args& f) {
        return launch_fft_list(ctx, f, t2->ep_drs.as<uint16_t>(), t2->n_ep_drs, p.n, st);
    };
    int err = tracked_pass(ctx, p, p.t->pcc_max + 1, t2->q.N_DF_symb, fa, st, drs_pass, drs_pass);
    if (err == DNRP_OK) err = launch_snr_chain(ctx, p, st);
    if (err != DNRP_OK) return err;
    dev::rx_epoch_args x{};
    x.F = fa;
    x.C = ca;
    if (t2->eplan_ok) {
        x.C.epochs = t2->eplan.epochs.as<dev::rx_epoch>();
        x.C.segs = t2->eplan.segs.as<dev::rx_seg>();
    }
    x.ep_off = t2->ep_off.as<uint16_t>();
    x.ep_sym = t2->ep_sym.as<uint16_t>();
    ctx->tic("rx_epoch", st);
    if (dev::launch_rx_epoch(x, p.n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("rx_epoch", st);
    return DNRP_OK;
}

// packet groups: front end of group g on st, back end of group g on rx_aux once that front end is
// done, so group g+1's front end runs beside group g's back end and the back end reads Y (plain
// stores) while it is still in the L2 / Infinity Cache. Every front end takes it (each launch selects
// its packets through sel); y_plain is read by the streaming wave kernel only (N_b_DFT_os = 1024),
// the others store as ever
int pdc_grouped_y(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, dev::rx_front_args fa, hipStream_t st) {
    if (!ctx->rx_aux) {
        HIPCHK(hipStreamCreateWithFlags(&ctx->rx_aux, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ctx->rx_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ctx->rx_join, hipEventDisableTiming));
    }
    const uint32_t G = ctx->sw.rx_group;
    fa.sym_count = t2->q.N_DF_symb - p.t->pcc_max;
    fa.y_plain = 1;
    ctx->tic("rx_pdc_phase", st);  // both streams' launches of the phase, fork to join
    for (uint32_t g0 = 0; g0 < p.n; g0 += G) {
        rx_phase pg = p;
        pg.n = std::min(G, p.n - g0);
        pg.sel = p.sel + 2 * g0;
        fa.sel = pg.sel;
        ctx->tic("rx_fft_pdc", st);
        if (dev::launch_rx_fft(fa, pg.n, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("rx_fft_pdc", st);
        HIPCHK(hipEventRecord(ctx->rx_fork, st));
        HIPCHK(hipStreamWaitEvent(ctx->rx_aux, ctx->rx_fork, 0));
        const auto cg = cells_args(ctx, pg);
        const int err = launch_back(ctx, pg, &cg, ctx->rx_aux);
        if (err != DNRP_OK) return err;
    }
    HIPCHK(hipEventRecord(ctx->rx_join, ctx->rx_aux));
    HIPCHK(hipStreamWaitEvent(st, ctx->rx_join, 0));
    ctx->toc("rx_pdc_phase", st);
    return DNRP_OK;
}

int pdc_plain_y(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, dev::rx_front_args fa,
                const dev::rx_cells_args& ca, hipStream_t st) {
    if (t2->q.N_DF_symb > p.t->pcc_max) {
        fa.sym_count = t2->q.N_DF_symb - p.t->pcc_max;
        const int err = tracked_pass(
            ctx, p, p.t->pcc_max + 1, t2->q.N_DF_symb, fa, st,
            [&](const dev::rx_front_args& f) {  // the phase's DRS symbols: the plan's ops behind the PCC phase's
                const uint32_t d0 = p.t->bplan.n_dops, nd = p.plan->n_dops - d0;
                return launch_fft_list(ctx, f, p.plan->dl16.as<uint16_t>() + d0, nd, p.n, st, p.plan->dl_h.data() + d0);
            },
            [&](const dev::rx_front_args& f) {
                ctx->tic("rx_fft_pdc", st);
                if (dev::launch_rx_fft(f, p.n, st) != hipSuccess) return DNRP_EDEVICE;
                ctx->toc("rx_fft_pdc", st);
                return DNRP_OK;
            });
        if (err != DNRP_OK) return err;
    }
    return launch_back(ctx, p, &ca, st);
}

// MIMO report at the packet end (rx_synced.cpp:417-436; the reference runs it after a successful CRC,
// which is the caller's decision here). fa.zd set: the fused receiver ran, the DRS bins of this phase
// are not in Y and the pilots hold the same values
dev::rx_mimo_args mimo_args(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, const dev::rx_front_args& fa) {
    dev::rx_mimo_args ma{};
    ma.N_RX = ctx->cfg.N_TX_max;
    ma.N_TS = t2->N_TS;
    ma.Nf_pad = ctx->rx_Nf_pad;
    ma.n_sym_total = ctx->rx_nsym_cap + 1;
    ma.ncb_tx = t2->ncb_tx;
    ma.A_tx = t2->A_tx;
    ma.ncb_rx = t2->ncb_rx;
    ma.A_rx = t2->A_rx;
    ma.cells = t2->mimo_cells.as<uint32_t>();
    ma.signs = t2->mimo_signs.as<float>();
    ma.Wtx = t2->Wtx.as<float2>();
    ma.stx = t2->stx.as<float>();
    ma.Wrx = t2->Wrx.as<float2>();
    ma.srx = t2->srx.as<float>();
    ma.Y = ctx->Y.as<float2>();
    ma.out = ctx->mimo_out.as<uint32_t>();
    ma.sel = p.sel;
    if (fa.zd) {
        ma.zd = fa.zd;
        ma.zcells = t2->mimo_zcells.as<uint32_t>();
        ma.zd_dops = fa.zd_dops;
        ma.zd_row = fa.zd_row;
    }
    return ma;
}

int pdc_mimo(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, const dev::rx_front_args& fa, hipStream_t st) {
    return dev::launch_rx_mimo(mimo_args(ctx, p, t2, fa), p.n, st) == hipSuccess ? DNRP_OK : DNRP_EDEVICE;
}

// the same report through rx_mimo_detail_kernel under a non-default dnrp_ctx_set_rx_mimo_report (o: what the
// PDC call read of it): the chosen metric and search start, every score, the rank / precoder report. The
// noise variance is the nv_d entry of the phase's last DRS op, which rx_snr_kernel writes on every PDC path
// (launch_back and launch_snr_chain run it over all of the plan's ops for all of the group's packets; the
// grouped Y path's auxiliary stream has joined st by now)
struct mimo_opts {
    uint32_t metric = 0, all_w = 0, detail = 0;
    bool on() const { return metric || all_w || detail; }
};

static_assert(sizeof(dev::rx_mimo_detail_row) == sizeof(dnrp_mimo_detail), "dnrp_mimo_detail layout");
static_assert(dev::RX_MIMO_MAX_CB == DNRP_MIMO_MAX_CB, "DNRP_MIMO_MAX_CB");

int pdc_mimo_detail(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, const dev::rx_front_args& fa,
                    const mimo_opts& o, hipStream_t st) {
    dev::rx_mimo_detail_args da{};
    da.M = mimo_args(ctx, p, t2, fa);
    if (o.all_w) da.M.A_tx = da.M.A_rx = 0;
    da.metric = o.metric;
    da.n_dops = p.plan->n_dops;
    da.nv_d = ctx->nv_d.as<float>();
    for (int s = 0; s < 3; ++s) {
        da.sm_ncb[s] = t2->sm_ncb[s];
        da.sm_woff[s] = t2->sm_woff[s];
        da.sm_cboff[s] = t2->sm_cboff[s];
    }
    da.Wsm = t2->Wsm.as<float2>();
    da.ssm = t2->ssm.as<float>();
    da.rows = ctx->mimo_rows.as<dev::rx_mimo_detail_row>();
    ctx->tic("rx_mimo_detail", st);
    if (dev::launch_rx_mimo_detail(da, p.n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("rx_mimo_detail", st);
    return DNRP_OK;
}

static_assert(sizeof(dev::rx_aoa_row) == sizeof(dnrp_aoa_report) && offsetof(dev::rx_aoa_row, n_cells) == offsetof(dnrp_aoa_report, n_cells) &&
                  offsetof(dev::rx_aoa_row, az_rad) == offsetof(dnrp_aoa_report, az_rad) &&
                  offsetof(dev::rx_aoa_row, lag_re) == offsetof(dnrp_aoa_report, lag_re) &&
                  offsetof(dev::rx_aoa_row, reserved) == offsetof(dnrp_aoa_report, reserved),
              "dnrp_aoa_report layout");

// the angle-of-arrival report of a launch group under the setting s the PDC call read: every DRS row of the
// packet is in Y behind any receiver but the fused one, which is not chosen then (the grouped Y path's auxiliary
// stream has joined st by now)
int pdc_aoa(dnrp_ctx* ctx, const rx_phase& p, const dnrp_ctx::aoa_setting& s, hipStream_t st) {
    dev::rx_aoa_args a{};
    a.V = drs_view(ctx, p);
    a.steer = s.steer.as<double2>();
    a.n_grid = s.grid.n_grid;
    a.cyclic = s.grid.cyclic;
    a.az0 = s.grid.az0;
    a.step = s.grid.step;
    a.rows = ctx->aoa_rows.as<dev::rx_aoa_row>();
    ctx->tic("rx_aoa", st);
    if (dev::launch_rx_aoa(a, p.n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("rx_aoa", st);
    return DNRP_OK;
}

// one launch group of the PDC call: its receiver, then the MIMO report where the caller asked for reports (or,
// with the detailed report on, for its rows), then the angle-of-arrival report where that setting is on
int pdc_group(dnrp_ctx* ctx, const rx_phase& p, const rx2_tables* t2, const float* iq_in, bool mimo, const mimo_opts& mo,
              const dnrp_ctx::aoa_setting* aoa, hipStream_t st) {
    auto fa = front_args(ctx, p.t, iq_in, p.sel, snr_from_front(ctx, p.t) ? p.plan : nullptr);
    const auto ca = cells_args(ctx, p);
    const pdc_path path = choose_pdc_path(ctx->sw, p.t, t2, fa, ca, p.n, rx_tracking(ctx), aoa != nullptr);
    if (rx_tracking(ctx)) {  // the PCC plan's ops are the PDC plan's ops up to pcc_max: the state continues there
        uint32_t d0 = 0;
        while (d0 < p.plan->n_dops && p.plan->dl_h[d0] <= p.t->pcc_max) ++d0;
        if (d0 != p.t->bplan.n_dops) return DNRP_EUNSUPPORTED;
    }
    if (path != pdc_path::fused) {
        fa.zd = nullptr;  // no reader
        fa.sym_first = p.t->pcc_max + 1;
    }
    int err = DNRP_OK;
    switch (path) {
        case pdc_path::fused: err = pdc_fused(ctx, p, t2, fa, st); break;
        case pdc_path::epoch: err = pdc_epoch(ctx, p, t2, fa, ca, st); break;
        case pdc_path::grouped_y: err = pdc_grouped_y(ctx, p, t2, fa, st); break;
        case pdc_path::plain_y: err = pdc_plain_y(ctx, p, t2, fa, ca, st); break;
    }
    if (err == DNRP_OK && mimo) err = mo.on() ? pdc_mimo_detail(ctx, p, t2, fa, mo, st) : pdc_mimo(ctx, p, t2, fa, st);
    if (err == DNRP_OK && aoa) err = pdc_aoa(ctx, p, *aoa, st);
    return err;
}

// the PDC reports of the call: the SNR chain's PDC estimate and the MIMO report of every request
int pdc_reports(dnrp_ctx* ctx, uint32_t m, const dnrp_pdc_req* req, dnrp_pdc_report* rep, hipStream_t st) {
    std::vector<dev::rx_pkt_state> S(ctx->rx_n);
    std::vector<uint32_t> mo(3 * size_t(m));
    HIPCHK(hipMemcpyAsync(S.data(), ctx->rx_st.p, sizeof(dev::rx_pkt_state) * ctx->rx_n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mo.data(), ctx->mimo_out.p, mo.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t r = 0; r < m; ++r) {
        rep[r].snr_dB = S[req[r].pcc_index].snr_pdc;
        rep[r].mimo_N_RX = ctx->cfg.N_TX_max;
        rep[r].mimo_N_TS_other = mo[3 * r];
        rep[r].tm_3_7_beamforming_idx = mo[3 * r + 1];
        rep[r].tm_3_7_beamforming_reciprocal_idx = mo[3 * r + 2];
    }
    return DNRP_OK;
}

}  // namespace

namespace {

// the two residual tracking settings (dnrp_ctx_set_rx_sto_tracking, dnrp_ctx_set_rx_cfo_tracking) and their tables
int set_tracking(uint32_t& to_on, float& to_gain, uint32_t on, float gain) {
    if (on > 1 || !std::isfinite(gain) || gain < 0.0f || gain > 1.0f) return DNRP_EINVAL;
    to_on = on;
    to_gain = gain;
    return DNRP_OK;
}

int get_tracking(uint32_t from_on, float from_gain, uint32_t* on, float* gain) {
    if (on) *on = from_on;
    if (gain) *gain = from_gain;
    return DNRP_OK;
}

// the common part of the table read-backs: *n_sym, and the table rows to copy (the device selected), 0
// (DNRP_OK) for a size query, or an error
int track_rows(dnrp_ctx* ctx, bool on, bool copy, uint32_t n_slots, uint32_t n_sym_cap, uint32_t* n_sym) {
    if (!ctx || !n_sym || !ctx->rx_valid || !on) return DNRP_EINVAL;
    *n_sym = ctx->rx_nsym_cap + 1;
    if (!copy) return DNRP_OK;
    if (n_slots == 0 || n_slots > ctx->rx_n || n_sym_cap < *n_sym) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    return static_cast<int>(n_slots * *n_sym);
}

}  // namespace

// ---- the angle-of-arrival setting: validation, azimuth grid and steering table (dnrp.h dnrp_ctx_set_rx_aoa)
namespace {
constexpr double AOA_TWO_PI = 6.283185307179586476925, AOA_SPAN_TOL = 1e-5;
}

bool dnrp::host::aoa_cfg_ok(const dnrp_aoa_cfg* cfg) {
    for (int r = 0; r < 8; ++r)
        if (!std::isfinite(cfg->pos[r][0]) || !std::isfinite(cfg->pos[r][1])) return false;
    if (!std::isfinite(cfg->az_min) || !std::isfinite(cfg->az_max)) return false;
    const double span = static_cast<double>(cfg->az_max) - static_cast<double>(cfg->az_min);
    return span > 0.0 && span <= AOA_TWO_PI + AOA_SPAN_TOL && cfg->n_grid >= 8 && cfg->n_grid <= dev::RX_AOA_MAX_GRID &&
           cfg->reserved == 0;
}

aoa_grid dnrp::host::aoa_grid_of(const dnrp_aoa_cfg& cfg) {
    const double span = static_cast<double>(cfg.az_max) - static_cast<double>(cfg.az_min);
    aoa_grid g;
    g.n_grid = cfg.n_grid;
    g.cyclic = std::fabs(span - AOA_TWO_PI) <= AOA_SPAN_TOL ? 1u : 0u;
    g.az0 = cfg.az_min;
    g.step = g.cyclic ? AOA_TWO_PI / cfg.n_grid : span / (cfg.n_grid - 1);
    return g;
}

std::vector<double2> dnrp::host::aoa_steering(const dnrp_aoa_cfg& cfg, const aoa_grid& g, uint32_t N_RX) {
    std::vector<double2> s(size_t(g.n_grid) * N_RX);
    for (uint32_t i = 0; i < g.n_grid; ++i) {
        const double az = g.az0 + i * g.step, c = std::cos(az), sn = std::sin(az);
        for (uint32_t r = 0; r < N_RX; ++r) {
            const double ph = AOA_TWO_PI * (static_cast<double>(cfg.pos[r][0]) * c + static_cast<double>(cfg.pos[r][1]) * sn);
            s[size_t(i) * N_RX + r] = make_double2(std::cos(ph), std::sin(ph));
        }
    }
    return s;
}

extern "C" {

int dnrp_rx_pcc_batch(dnrp_ctx* ctx, uint32_t n, const dnrp_sync_report* sr, const float* iq_in, uint32_t n_windows,
                      uint32_t S_in, int16_t* pcc_llr, dnrp_pcc_report* rep, void* stream) {
    if (!ctx || (n > 0 && (!sr || !iq_in || !pcc_llr))) return DNRP_EINVAL;
    ctx->rx_valid = false;
    if (n == 0) return DNRP_OK;
    if (n > ctx->cfg.max_batch) return DNRP_ENOMEM;
    (void)hipSetDevice(ctx->cfg.device);
    // packets grouped by (u, b, N_eff_TX) of their sync report: one launch set per group, each
    // packet processed exactly as an independent demoddecod_rx_pcc call (rx_synced.cpp:186-323)
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::vector<uint32_t>> groups;
    for (uint32_t i = 0; i < n; ++i) {
        if (sr[i].fine_peak_time >= static_cast<int64_t>(S_in) || sr[i].fine_peak_time <= -static_cast<int64_t>(S_in))
            return DNRP_EINVAL;
        if (sr[i].window >= n_windows) return DNRP_EINVAL;  // the kernels read iq_in + window * N_RX * S_in
        groups[std::make_tuple(sr[i].u, sr[i].b, sr[i].N_eff_TX)].push_back(i);
    }
    int err = DNRP_OK;
    const uint64_t dect = uint64_t(S_in) * ctx->cfg.M / ctx->cfg.L;  // DECT-rate samples in the window
    std::vector<std::pair<rx1_tables*, const std::vector<uint32_t>*>> gl;
    uint32_t cap_max = 0, nf_max = 0;
    ctx->rx_slot_t.assign(n, nullptr);
    ctx->rx_slot_cap.assign(n, 0);
    for (const auto& g : groups) {
        rx1_tables* t = get_rx1(ctx, std::get<0>(g.first), std::get<1>(g.first), std::get<2>(g.first), &err);
        if (!t) return err;
        // symbols that fit into the window: (S_in * M/L - STF) / symbol
        const uint64_t n_stf = t->STF_CP + t->Nd;
        if (dect < n_stf + t->CP + t->Nd) return DNRP_EINVAL;
        const uint32_t cap = static_cast<uint32_t>((dect - n_stf) / (t->CP + t->Nd));
        if (cap < t->pcc_max) return DNRP_EINVAL;
        cap_max = std::max(cap_max, cap);
        nf_max = std::max(nf_max, (t->N_occ + 1 + 63) / 64 * 64);
        for (uint32_t i : g.second) {
            ctx->rx_slot_t[i] = t;
            ctx->rx_slot_cap[i] = cap;
        }
        gl.emplace_back(t, &g.second);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    ctx->rx_nsym_cap = cap_max;
    ctx->rx_Nf_pad = nf_max;
    ctx->rx_S_in = S_in;
    ctx->rx_n = n;
    ctx->rx_iq = iq_in;
    ctx->rx_n_windows = n_windows;
    const size_t ybytes = size_t(n) * ctx->cfg.N_TX_max * (ctx->rx_nsym_cap + 1) * ctx->rx_Nf_pad * sizeof(float2);
    const size_t pbytes = size_t(n) * (ctx->rx_nsym_cap + 1) * ctx->cfg.N_TX_max * 8 * sizeof(double2);
    if (!ctx->Y.ensure(ybytes) || !ctx->snr_part.ensure(pbytes) || !ctx->rx_in.ensure(sizeof(dev::rx_pkt_in) * ctx->cfg.max_batch) ||
        !ctx->rx_st.ensure(sizeof(dev::rx_pkt_state) * ctx->cfg.max_batch) ||
        !ctx->rx_sel.ensure(2 * sizeof(uint32_t) * ctx->cfg.max_batch) ||
        !ctx->stf_part.ensure(size_t(ctx->cfg.max_batch) * 8 * (sizeof(double2) + sizeof(float) + 14 * ctx->cfg.b_max * sizeof(float2))) ||
        !ctx->lut_d.ensure(size_t(ctx->cfg.max_batch) * dev::RX_MAX_DOPS) ||
        !ctx->nv_d.ensure(size_t(ctx->cfg.max_batch) * dev::RX_MAX_DOPS * sizeof(float)))
        return DNRP_ENOMEM;
    read_pcc(ctx->sw);  // once per PCC call: its PDC call takes the same switches
    ctx->rx_sto_on = ctx->sto_track_on != 0;  // likewise the residual STO tracking setting
    ctx->rx_sto_gain = ctx->sto_track_gain;
    if (ctx->rx_sto_on) {  // the per-symbol table, NaN (all bits set) until a phase fills its symbols
        const size_t tbytes = size_t(n) * (ctx->rx_nsym_cap + 1) * sizeof(double);
        if (!ctx->sto_sym.ensure(tbytes)) return DNRP_ENOMEM;
        HIPCHK(hipMemsetAsync(ctx->sto_sym.p, 0xFF, tbytes, st));
    }
    ctx->rx_cfo_on = ctx->cfo_track_on != 0;  // and the residual CFO tracking setting
    ctx->rx_cfo_gain = ctx->cfo_track_gain;
    if (ctx->rx_cfo_on) {  // its table likewise, and the PCC phase's pilots
        const size_t tbytes = size_t(n) * (ctx->rx_nsym_cap + 1) * sizeof(double2);
        const size_t kbytes = size_t(n) * dev::RX_CFO_KEEP * ctx->cfg.N_TX_max * 14 * ctx->cfg.b_max * 4 * sizeof(float2);
        if (!ctx->cfo_sym.ensure(tbytes) || !ctx->cfo_keep.ensure(kbytes)) return DNRP_ENOMEM;
        HIPCHK(hipMemsetAsync(ctx->cfo_sym.p, 0xFF, tbytes, st));
    }
    {
        // zero-forced DRS pilots of every slot (the fused receiver's only): at most one DRS symbol per
        // 5 symbols (N_eff_TX <= 4) plus the zero op
        ctx->zd_row = 14 * ctx->cfg.b_max;
        ctx->zd_dops = std::min<uint32_t>(dev::RX_MAX_DOPS, (cap_max + 4) / 5 + 2) + 1;
        const size_t zbytes = size_t(n) * ctx->zd_dops * ctx->cfg.N_TX_max * 4 * ctx->zd_row * sizeof(float2);
        if (ctx->sw.rx_fused) {
            if (!ctx->zd.ensure(zbytes)) return DNRP_ENOMEM;
            // the size is part of the key: a reallocation can return the same base address
            const auto key = std::make_tuple(ctx->zd.p, ctx->zd.n, ctx->zd_dops, ctx->zd_row, ctx->cfg.N_TX_max);
            if (key != ctx->zd_key) {  // a new layout: the zero op of every slot (and all else) zeroed once
                HIPCHK(hipMemsetAsync(ctx->zd.p, 0, ctx->zd.n, st));
                ctx->zd_key = key;
            }
        }
    }
    auto* pin = static_cast<dev::rx_pkt_in*>(ctx->st_rxin.get(sizeof(dev::rx_pkt_in) * n));
    auto* sel = static_cast<uint32_t*>(ctx->st_sel.get(2 * sizeof(uint32_t) * n));
    if (!pin || !sel) return DNRP_ENOMEM;
    for (uint32_t i = 0; i < n; ++i) {
        pin[i].fine_peak = sr[i].fine_peak_time;
        pin[i].cfo_rad = sr[i].cfo_fractional_rad + sr[i].cfo_integer_rad;
        pin[i].inc0 = phasor_arg(pin[i].cfo_rad);
        pin[i].win = sr[i].window;
    }
    {
        uint32_t o = 0;
        for (const auto& g : gl)
            for (uint32_t i : *g.second) {
                sel[2 * o] = i;
                sel[2 * o + 1] = i;  // PCC LLR row = slot
                ++o;
            }
    }
    HIPCHK(hipMemcpyAsync(ctx->rx_in.p, pin, sizeof(dev::rx_pkt_in) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_rxin.ev, st));
    HIPCHK(hipMemcpyAsync(ctx->rx_sel.p, sel, 2 * sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_sel.ev, st));
    uint32_t off = 0;
    for (const auto& g : gl) {
        rx1_tables* t = g.first;
        const uint32_t ng = static_cast<uint32_t>(g.second->size());
        const uint32_t* gsel = ctx->rx_sel.as<uint32_t>() + 2 * off;
        off += ng;
        auto fa = front_args(ctx, t, iq_in, gsel, snr_from_front(ctx, t) ? &t->bplan : nullptr);
        ctx->tic("rx_stf", st);
        if (dev::launch_rx_stf(fa, ng, st) != hipSuccess) return DNRP_EDEVICE;
        ctx->toc("rx_stf", st);
        fa.sym_first = 1;
        fa.sym_count = t->pcc_max;
        const rx_phase p{t, &t->bplan, ng, gsel, false, 2, t->pcc_k.as<uint32_t>(), t->pcc_sym.as<uint16_t>(), pcc_llr, 196, false};
        // residual STO / CFO tracking: the phase's few symbols with the STF values, the tables from their DRS
        // rows, then the same launch again with the tables
        auto fft_pcc = [&](const dev::rx_front_args& f) {
            ctx->tic("rx_fft_pcc", st);
            if (dev::launch_rx_fft(f, ng, st) != hipSuccess) return DNRP_EDEVICE;
            ctx->toc("rx_fft_pcc", st);
            return DNRP_OK;
        };
        err = tracked_pass(ctx, p, 0, t->pcc_max, fa, st, fft_pcc, fft_pcc);
        if (err != DNRP_OK) return err;
        const auto ca = cells_args(ctx, p);
        err = launch_back(ctx, p, &ca, st);
        if (err != DNRP_OK) return err;
    }
    ctx->rx_valid = true;
    if (rep) {
        std::vector<dev::rx_pkt_state> S(n);
        HIPCHK(hipMemcpyAsync(S.data(), ctx->rx_st.p, sizeof(dev::rx_pkt_state) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < n; ++i) {
            rep[i].snr_dB = S[i].snr_pcc;
            rep[i].cfo_fractional_rad = sr[i].cfo_fractional_rad + (S[i].cfo_fine - pin[i].cfo_rad);
            rep[i].sto_fractional = S[i].sto_frac;
            // run_stf_rms_estimation (rx_synced.cpp:620-655): sync's RMS kept where it is > 0
            for (int a = 0; a < 8; ++a)
                rep[i].rms[a] = (prm::RX_RMS_KEEP_SYNC && sr[i].rms[a] > 0.0f) ? sr[i].rms[a] : S[i].rms[a];
        }
    }
    return DNRP_OK;
}

int dnrp_rx_pdc_batch(dnrp_ctx* ctx, uint32_t m, const dnrp_pdc_req* req, const float* iq_in, uint32_t n_windows,
                      uint32_t S_in, int16_t* pdc_llr, uint32_t llr_stride, dnrp_pdc_report* rep, void* stream) {
    if (!ctx || (m > 0 && (!req || !iq_in || !pdc_llr))) return DNRP_EINVAL;
    // no packet continues with its PDC: nothing to enqueue, whatever the PCC call before (an empty
    // chunk enqueues no job either, worker_sync.cpp:170-190)
    if (m == 0) return DNRP_OK;
    if (!ctx->rx_valid) return DNRP_ESTATE;
    // the PDC symbols are read from the PCC call's windows (the state it kept points into them)
    if (iq_in != ctx->rx_iq || n_windows != ctx->rx_n_windows) return DNRP_ESTATE;
    if (m > ctx->rx_n || S_in != ctx->rx_S_in) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    int err = DNRP_OK;
    // requests grouped by (PCC-phase tables, PLCF-announced psdef) (rx_synced.cpp:325-436 per packet)
    using key_t = std::tuple<rx1_tables*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>;
    std::map<key_t, std::vector<uint32_t>> groups;
    std::vector<uint8_t> seen(ctx->rx_n, 0);
    for (uint32_t r = 0; r < m; ++r) {
        const auto& q = req[r];
        if (q.pcc_index >= ctx->rx_n || seen[q.pcc_index]) return DNRP_EINVAL;
        seen[q.pcc_index] = 1;
        if (q.plcf_type != 1 && q.plcf_type != 2) return DNRP_EINVAL;
        const auto& d = q.psdef;
        groups[key_t(ctx->rx_slot_t[q.pcc_index], d.u, d.b, d.PacketLengthType, d.PacketLength, d.tm_mode_index,
                     d.mcs_index, d.Z)]
            .push_back(r);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!ctx->pdc_seq_ptrs.ensure(sizeof(void*) * ctx->cfg.max_batch) ||
        !ctx->rx_sel2.ensure(2 * sizeof(uint32_t) * ctx->cfg.max_batch))
        return DNRP_ENOMEM;
    auto** seqp = static_cast<const uint8_t**>(ctx->st_seq.get(sizeof(void*) * m));
    auto* sel = static_cast<uint32_t*>(ctx->st_sel2.get(2 * sizeof(uint32_t) * m));
    if (!seqp || !sel) return DNRP_ENOMEM;
    std::vector<std::pair<rx2_tables*, const std::vector<uint32_t>*>> gl;
    uint32_t o = 0;
    for (const auto& g : groups) {
        rx1_tables* t = std::get<0>(g.first);
        const dnrp_psdef& d = req[g.second.front()].psdef;
        rx2_tables* t2 = get_rx2(ctx, d, &err);
        if (!t2) return err;
        if (d.u != t->u || d.b != t->b || t2->q.N_eff_TX != t->N_eff_TX) return DNRP_EINVAL;
        if (rx_tracking(ctx) && t2->sm) return DNRP_EUNSUPPORTED;  // the MMSE receiver has no tracking; nothing launched yet
        if (llr_stride < t2->q.G) return DNRP_EINVAL;
        for (uint32_t r : g.second) {
            if (t2->q.N_DF_symb > ctx->rx_slot_cap[req[r].pcc_index]) return DNRP_EINVAL;
            auto it = ctx->netid.find(req[r].network_id);
            if (it == ctx->netid.end()) return DNRP_ENETID;
            err = ensure_seq(ctx, *it->second, req[r].network_id, t2->q.G);
            if (err != DNRP_OK) return err;
            seqp[r] = (req[r].plcf_type == 1 ? it->second->t1 : it->second->t2).as<uint8_t>();
            sel[2 * o] = req[r].pcc_index;
            sel[2 * o + 1] = r;
            ++o;
        }
        gl.emplace_back(t2, &g.second);
    }
    HIPCHK(hipMemcpyAsync(ctx->pdc_seq_ptrs.p, seqp, sizeof(void*) * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_seq.ev, st));
    HIPCHK(hipMemcpyAsync(ctx->rx_sel2.p, sel, 2 * sizeof(uint32_t) * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_sel2.ev, st));
    // the MIMO report options, read once per call: the default runs rx_mimo_kernel where the caller takes reports,
    // as ever; any other setting runs rx_mimo_detail_kernel there, and with detail = 1 for its rows alone too
    const mimo_opts mo{ctx->mimo_metric, ctx->mimo_all_w, ctx->mimo_detail};
    const bool mimo = rep != nullptr || mo.detail != 0;
    ctx->mimo_rows_m = 0;
    if (mimo && !ctx->mimo_out.ensure(size_t(ctx->cfg.max_batch) * 3 * sizeof(uint32_t))) return DNRP_ENOMEM;
    if (mimo && mo.on() && !ctx->mimo_rows.ensure(size_t(ctx->cfg.max_batch) * sizeof(dnrp_mimo_detail))) return DNRP_ENOMEM;
    // the angle-of-arrival setting likewise: this call's launches keep the object they took here
    ctx->aoa_rows_m = 0;
    if (ctx->aoa_used != ctx->aoa) ctx->aoa_used = ctx->aoa;
    const dnrp_ctx::aoa_setting* aoa = ctx->aoa_used.get();
    if (aoa && !ctx->aoa_rows.ensure(size_t(ctx->cfg.max_batch) * sizeof(dnrp_aoa_report))) return DNRP_ENOMEM;
    uint32_t off = 0;
    size_t gi = 0;
    for (const auto& g : groups) {
        rx1_tables* t = std::get<0>(g.first);
        rx2_tables* t2 = gl[gi++].first;
        const uint32_t ng = static_cast<uint32_t>(g.second.size());
        const uint32_t* gsel = ctx->rx_sel2.as<uint32_t>() + 2 * off;
        off += ng;
        const rx_phase p{t, &t2->bplan, ng, gsel, true, t2->q.N_bps, t2->pdc_k.as<uint32_t>(), t2->pdc_sym.as<uint16_t>(),
                         pdc_llr, llr_stride, t2->sm};
        err = pdc_group(ctx, p, t2, iq_in, mimo, mo, aoa, st);
        if (err != DNRP_OK) return err;
    }
    if (mo.detail) ctx->mimo_rows_m = m;
    if (aoa) ctx->aoa_rows_m = m;
    return rep ? pdc_reports(ctx, m, req, rep, st) : DNRP_OK;
}

int dnrp_ctx_set_rx_mimo_report(dnrp_ctx* ctx, uint32_t metric, uint32_t all_w, uint32_t detail) {
    if (!ctx || metric > DNRP_MIMO_METRIC_MIN_SPREAD_RX_POWER || all_w > 1 || detail > 1) return DNRP_EINVAL;
    ctx->mimo_metric = metric;
    ctx->mimo_all_w = all_w;
    ctx->mimo_detail = detail;
    return DNRP_OK;
}

int dnrp_ctx_get_rx_mimo_report(const dnrp_ctx* ctx, uint32_t* metric, uint32_t* all_w, uint32_t* detail) {
    if (!ctx) return DNRP_EINVAL;
    if (metric) *metric = ctx->mimo_metric;
    if (all_w) *all_w = ctx->mimo_all_w;
    if (detail) *detail = ctx->mimo_detail;
    return DNRP_OK;
}

int dnrp_rx_mimo_detail(dnrp_ctx* ctx, uint32_t m, dnrp_mimo_detail* out, void* stream) {
    if (!ctx || !out || m == 0) return DNRP_EINVAL;
    if (!ctx->mimo_rows_m) return DNRP_ESTATE;
    if (m > ctx->mimo_rows_m) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(hipMemcpyAsync(out, ctx->mimo_rows.p, size_t(m) * sizeof(dnrp_mimo_detail), hipMemcpyDeviceToHost,
                          static_cast<hipStream_t>(stream)));
    return DNRP_OK;
}

int dnrp_ctx_set_rx_aoa(dnrp_ctx* ctx, const dnrp_aoa_cfg* cfg) {
    if (!ctx) return DNRP_EINVAL;
    if (!cfg) {
        ctx->aoa.reset();
        return DNRP_OK;
    }
    if (ctx->cfg.N_TX_max < 2 || !aoa_cfg_ok(cfg)) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    auto s = std::make_shared<dnrp_ctx::aoa_setting>();
    s->cfg = *cfg;
    s->grid = aoa_grid_of(*cfg);
    if (!s->steer.upload(aoa_steering(*cfg, s->grid, ctx->cfg.N_TX_max))) return DNRP_ENOMEM;
    ctx->aoa = std::move(s);
    return DNRP_OK;
}

int dnrp_ctx_get_rx_aoa(const dnrp_ctx* ctx, uint32_t* on, dnrp_aoa_cfg* cfg) {
    if (!ctx) return DNRP_EINVAL;
    if (on) *on = ctx->aoa ? 1u : 0u;
    if (cfg && ctx->aoa) *cfg = ctx->aoa->cfg;
    return DNRP_OK;
}

int dnrp_rx_aoa(dnrp_ctx* ctx, uint32_t m, dnrp_aoa_report* out, void* stream) {
    if (!ctx || !out || m == 0) return DNRP_EINVAL;
    if (!ctx->aoa_rows_m) return DNRP_ESTATE;
    if (m > ctx->aoa_rows_m) return DNRP_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(hipMemcpyAsync(out, ctx->aoa_rows.p, size_t(m) * sizeof(dnrp_aoa_report), hipMemcpyDeviceToHost,
                          static_cast<hipStream_t>(stream)));
    return DNRP_OK;
}

int dnrp_aoa_estimate(const dnrp_aoa_cfg* cfg, uint32_t N_RX, const float* R, dnrp_aoa_report* out, float* spectrum) {
    if (!cfg || !R || !out || N_RX < 2 || N_RX > 8 || !aoa_cfg_ok(cfg)) return DNRP_EINVAL;
    const aoa_grid g = aoa_grid_of(*cfg);
    const std::vector<double2> steer = aoa_steering(*cfg, g, N_RX);
    const double tr = dev::aoa_trace(R, N_RX);
    std::vector<double> P(g.n_grid, 0.0);
    uint32_t best = 0;
    for (uint32_t i = 0; i < g.n_grid; ++i) {
        if (tr > 0.0) P[i] = dev::aoa_quad(R, steer.data() + size_t(i) * N_RX, N_RX) / (static_cast<double>(N_RX) * tr);
        if (P[i] > P[best]) best = i;
        if (spectrum) spectrum[i] = static_cast<float>(P[i]);
    }
    dev::rx_aoa_row row{};
    dev::aoa_finish(R, N_RX, P.data(), g.n_grid, g.cyclic, g.az0, g.step, tr, best, &row);
    out->grid_idx = row.grid_idx;
    out->az_rad = row.az_rad;
    out->peak = row.peak;
    out->lag_re = row.lag_re;
    out->lag_im = row.lag_im;
    out->reserved[0] = out->reserved[1] = 0;
    return DNRP_OK;
}

int dnrp_ctx_set_rx_sto_tracking(dnrp_ctx* ctx, uint32_t on, float gain) {
    return ctx ? set_tracking(ctx->sto_track_on, ctx->sto_track_gain, on, gain) : DNRP_EINVAL;
}

int dnrp_ctx_get_rx_sto_tracking(const dnrp_ctx* ctx, uint32_t* on, float* gain) {
    return ctx ? get_tracking(ctx->sto_track_on, ctx->sto_track_gain, on, gain) : DNRP_EINVAL;
}

int dnrp_rx_sto_track(dnrp_ctx* ctx, uint32_t n_slots, double* inc, uint32_t n_sym_cap, uint32_t* n_sym, void* stream) {
    const int rows = track_rows(ctx, ctx && ctx->rx_sto_on, inc != nullptr, n_slots, n_sym_cap, n_sym);
    if (rows <= 0) return rows;
    HIPCHK(hipMemcpyAsync(inc, ctx->sto_sym.p, size_t(rows) * sizeof(double), hipMemcpyDeviceToHost,
                          static_cast<hipStream_t>(stream)));
    return DNRP_OK;
}

int dnrp_ctx_set_rx_cfo_tracking(dnrp_ctx* ctx, uint32_t on, float gain) {
    return ctx ? set_tracking(ctx->cfo_track_on, ctx->cfo_track_gain, on, gain) : DNRP_EINVAL;
}

int dnrp_ctx_get_rx_cfo_tracking(const dnrp_ctx* ctx, uint32_t* on, float* gain) {
    return ctx ? get_tracking(ctx->cfo_track_on, ctx->cfo_track_gain, on, gain) : DNRP_EINVAL;
}

int dnrp_rx_cfo_track(dnrp_ctx* ctx, uint32_t n_slots, double* inc, double* phase, uint32_t n_sym_cap, uint32_t* n_sym,
                      void* stream) {
    const int rows = track_rows(ctx, ctx && ctx->rx_cfo_on, inc || phase, n_slots, n_sym_cap, n_sym);
    if (rows <= 0) return rows;
    // the device table holds (phase, increment) pairs: one strided copy per output array
    const auto* src = static_cast<const char*>(ctx->cfo_sym.p);
    if (phase)
        HIPCHK(hipMemcpy2DAsync(phase, sizeof(double), src, sizeof(double2), sizeof(double), rows, hipMemcpyDeviceToHost,
                                static_cast<hipStream_t>(stream)));
    if (inc)
        HIPCHK(hipMemcpy2DAsync(inc, sizeof(double), src + sizeof(double), sizeof(double2), sizeof(double), rows,
                                hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    return DNRP_OK;
}

}  // extern "C"
