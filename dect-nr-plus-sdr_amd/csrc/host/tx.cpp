// dnrp_tx_batch (include/dnrp.h): the argument block of one batched TX launch (kernels/tx.hip).
#include "ctx_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace {

// Window length of an N_b_DFT_os-point symbol (dft/windowing.cpp:34-39 with tx.cpp:71-77): the
// data-field cyclic prefix N_b_DFT_os / 8 times the fraction, rounded in float; 0: no valid window
uint32_t window_length(uint32_t N_b_DFT_os, float fraction) {
    if (N_b_DFT_os == 0 || N_b_DFT_os % 8 != 0 || !(fraction > 0.0f && fraction <= 1.0f)) return 0;
    const uint32_t N = static_cast<uint32_t>(std::round(static_cast<float>(N_b_DFT_os / 8) * fraction));
    return N >= 2 ? N : 0;
}

// rising edge (filter/raised_cosine.cpp:30-56), float arithmetic in the reference's order
std::vector<float> window_rising(uint32_t N) {
    std::vector<float> rc(N);
    const float N_f = static_cast<float>(N), pi_f = 3.14159265358979323846f;
    for (uint32_t n = 0; n < N; ++n) {
        const float A = std::cos((static_cast<float>(n) - N_f) / N_f * pi_f * 0.5f);
        rc[n] = A * A;
    }
    return rc;
}

// the window of a packet geometry at `fraction` (0: off): DNRP_OK with *win_n, or the error dnrp_tx_batch
// returns before anything is queued -- the reference asserts 2 <= N (dft/windowing.cpp:39)
int tx_window_n(const geo::dims_t& dm, const geo::resampler_t& rs, float fraction, uint32_t* win_n) {
    *win_n = 0;
    if (!(fraction > 0.0f)) return DNRP_OK;
    const uint32_t N = window_length(dm.Nd, fraction);
    if (N == 0) return dm.Nd % 8 ? DNRP_EUNSUPPORTED : DNRP_EINVAL;
    // tx.hip tx_window_run leaves the prefix of a run's history symbol unshaped: the resampler
    // history must end behind it
    if (N > dm.CP || rs.hl + N >= dm.CP + dm.Nd) return DNRP_EUNSUPPORTED;
    *win_n = N;
    return DNRP_OK;
}

// what the launch geometry of a packet configuration is computed from: host data alone (a context's
// tx_tables, or the geometry rebuilt without a device by dnrp_tx_form_for)
struct tx_geom {
    const dnrp_packet_sizes* q;
    const geo::tm_t* tm;
    const geo::dims_t* dm;
    const geo::resampler_t* rs;
    const uint32_t* pdc_off;   // [N_DF + 2] first PDC cell of each symbol
    const uint8_t* w_onehot;   // per codebook: one nonzero entry in every antenna row
    bool code_bin, code_oh;    // the streaming kernel's code tables exist (tables.cpp get_tx)
};

// Every value of the argument block that decides which kernel form launch_tx takes (dev::tx_form_of) and
// with which launch geometry, for n packets of one configuration into iq_out at address out_addr with row
// length S. Pure: no context, no device; the pointers of `a` stay unset.
void plan_tx(const tx_geom& t, const switches& sw, uint32_t n, const dnrp_tx_desc* desc, uint32_t S, uint32_t pdc_stride,
             uintptr_t out_addr, uint32_t win_n, dev::tx_args& a) {
    const auto& q = *t.q;
    const auto& tm = *t.tm;
    const auto& dm = *t.dm;
    const auto& rs = *t.rs;
    a.plan.N = dm.Nd;
    a.N_occ = q.N_b_OCC;
    a.off_lower = dm.off_lower;
    a.CP = dm.CP;
    a.STF_CP = dm.STF_CP;
    a.N_DF = q.N_DF_symb;
    a.N_TS = tm.N_TS;
    a.N_TX = tm.N_TX;
    a.N_SS = tm.N_SS;
    a.N_bps = q.N_bps;
    a.txdiv = tm.txdiv;
    fill_pairs(tm.N_TS, a.pair, a.mod);
    a.pattern_len = dm.pattern_len;
    a.L = rs.L;
    a.M = rs.M;
    a.delay = rs.delay;
    a.hl = rs.hl;
    a.n_keep = std::min(dm.N_no_GI_rs, S);
    a.S = S;
    a.pdc_stride = pdc_stride;
    a.G = q.G;
    a.win_n = win_n;
    // symbol runs (tx.hip): K symbols per WG plus the preceding symbol as resampler history
    // wave path (one wavefront per symbol slot): K = 6 symbols + history per 7-wave workgroup
    // (C4, 4096 slots per launch: K=3 12.3 ms, K=4 16.6, K=5 15.2, K=6 11.4, K=7 15.9 — LDS sets
    // 4 / 2 / 2 / 2 / 1 workgroups per CU); block path K = 3.
    const bool wave = dm.Nd == 1024;
    const uint32_t K = wave ? 6u : 3u;
    a.K = K;
    a.n_runs = (q.N_DF_symb + 1 + K - 1) / K;
    const auto al = geo::resampler_align(rs);
    a.m_star = al.m_star;
    a.p_star = al.p_star;
    a.HP = 2 * (rs.hl + rs.M + 1);
    {
        const uint32_t len0 = dm.STF_CP + dm.Nd, lenD = dm.CP + dm.Nd;
        auto bsym = [&](uint32_t l) { return l == 0 ? 0u : len0 + (l - 1) * lenD; };
        const uint32_t bpc = tm.N_SS * q.N_bps;
        uint32_t mx = 0, span = 0;
        for (uint32_t r = 0; r < a.n_runs; ++r) {
            const uint32_t lf = r * K, ll = std::min(lf + K, q.N_DF_symb + 1) - 1, s0 = std::max(lf, 1u) - 1;
            span = std::max(span, bsym(ll + 1) - bsym(s0));
            const uint64_t b0 = (uint64_t(t.pdc_off[std::max(s0, 1u)]) * bpc) >> 3;
            const uint64_t b1 = ((uint64_t(t.pdc_off[ll + 1]) * bpc + 7) >> 3) + 1;
            if (b1 > b0) mx = std::max<uint32_t>(mx, static_cast<uint32_t>(b1 - b0));
        }
        a.stage_bytes = mx <= 8192 ? (mx + 3) / 4 * 4 : 0;
        a.lin_len = std::max(2 * a.HP + span, (K + 1) * dm.Nd);
        // output staging reuses bufB + twiddles + constellation: size bufB for the longest run
        const uint32_t max_out = static_cast<uint32_t>((uint64_t(span + rs.hl) * rs.L + rs.M - 1) / rs.M) + rs.L;
        a.bufB_len = std::max((K + 1) * dm.Nd, max_out > dm.Nd + 256 ? max_out - dm.Nd - 256 : 0u);
    }
    if (dm.Nd > 1024) {
        // beyond the block path's registers (tx_kernel stages <= 4 bins per thread): the symbols go
        // through a DECT-rate scratch (tx.hip tx_big_sym_kernel), e.g. u < u_max at b_max = 16
        const uint64_t total = uint64_t(dm.STF_CP) + uint64_t(q.N_DF_symb) * dm.CP + uint64_t(q.N_DF_symb + 1) * dm.Nd;
        a.big_len = static_cast<uint32_t>((total + 3) / 4 * 4);
        // the scratch is capped at 4 GiB (sw.tx_big_cap): larger batches run in passes of big_batch packets (tx.hip)
        const uint64_t row_bytes = sizeof(float) * 2 * uint64_t(a.big_len) * tm.N_TX;
        a.big_batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(n, sw.tx_big_cap / row_bytes)));
        a.stage_bytes = 0;
    }
    // streaming kernel (tx.hip tx_stream_kernel) where its geometry holds (its windowed form holds a
    // window of up to CP = 128 samples)
    a.stream = 0;
    if (wave && t.code_bin && dev::tx_stream_taps_match(rs.h.data(), rs.h.size()) && a.L == 10 && a.M == 9 && a.hl == 22 && a.CP == 128 && a.STF_CP == 1280 &&
        a.pattern_len * 9 == a.STF_CP + 1024 && S % 2 == 0 && (out_addr & 15u) == 0 && q.G >= 121) {  // (a row of PDC bytes holds a 16-B load)
        // every symbol's PDC bytes (SFBC partners included) within its staging window: 1 KiB, spatial
        // multiplexing 4 KiB (tx.hip TXS_SBW_SM: its first KiB prefetched, the rest loaded per symbol)
        const uint32_t bpc = tm.N_SS * q.N_bps;
        const bool sm = tm.N_TS > 1 && !tm.txdiv;
        uint64_t span = 0;
        for (uint32_t l = 1; l <= q.N_DF_symb; ++l) {
            const uint64_t j0 = t.pdc_off[l] & ~1u, j1 = (uint64_t(t.pdc_off[l + 1]) + 1) & ~1ull;
            const uint64_t ab = ((j0 * bpc) >> 3) & ~15ull, hi = ((j1 * bpc + 7) >> 3) + 1;
            span = std::max(span, hi - ab);
        }
        const bool fits = span <= (sm ? 4096u : 1024u);
        a.sb_chunks = static_cast<uint32_t>((span + 1023) / 1024);
        const int qlo0 = -static_cast<int>((a.p_star + 8) / 9);
        const int64_t mfirst0 = int64_t(a.m_star) + 10 * qlo0;
        if (fits) {
            a.stream = 1;
            a.mfma = sw.tx_mfma;
            a.onehot = tm.N_TS > 1 && t.code_oh ? 1u : 0u;  // transmit diversity or spatial multiplexing
            for (uint32_t i = 0; i < n && a.onehot; ++i)
                a.onehot = t.w_onehot[desc[i].codebook_index] ? 1u : 0u;
            a.n_pieces = static_cast<uint32_t>((int64_t(a.n_keep) - mfirst0 + 1279) / 1280);
            // enough wavefronts for ~8 rounds of 16 per CU; each extra segment costs one history FFT
            const uint64_t per = uint64_t(n) * a.N_TX;
            uint32_t ns = static_cast<uint32_t>(std::min<uint64_t>((32768 + per - 1) / per, std::max(1u, a.n_pieces / 8)));
            a.n_seg = std::max(1u, ns);
            a.piece_per_seg = (a.n_pieces + a.n_seg - 1) / a.n_seg;
            a.n_seg = (a.n_pieces + a.piece_per_seg - 1) / a.piece_per_seg;
        }
    }
}

void export_form(const dev::tx_form& f, dnrp_tx_form* out) {
    out->family = f.family;
    out->L = f.L;
    out->M = f.M;
    out->hl = f.hl;
    out->windowed = f.windowed;
    out->mode = f.mode;
    out->q8 = f.q8;
    out->mfma = f.mfma;
    out->sb_chunks = f.sb_chunks;
    out->n_seg = f.n_seg;
    out->staged = f.staged;
    out->passes = f.passes;
}

}  // namespace

extern "C" int dnrp_tx_last_form(const dnrp_ctx* ctx, dnrp_tx_form* out) {
    if (!ctx || !out) return DNRP_EINVAL;
    if (!ctx->tx_form_valid) return DNRP_ESTATE;
    export_form(ctx->tx_form, out);
    return DNRP_OK;
}

extern "C" int dnrp_tx_form_for(const dnrp_cfg* cfg, const dnrp_psdef* psdef, uint32_t n, const uint32_t* codebook, uint32_t S,
                                uint32_t out_misalign, float win_fraction, dnrp_tx_form* out) {
    if (!cfg || !psdef || !out || n == 0 || !codebook || !(win_fraction >= 0.0f && win_fraction <= 1.0f)) return DNRP_EINVAL;
    dnrp_packet_sizes q{};
    geo::tm_t tm{};
    if (!geo::packet_sizes(*psdef, q, &tm)) return DNRP_ECONFIG;
    if (psdef->u > cfg->u_max || psdef->b > cfg->b_max || q.N_TX > cfg->N_TX_max || q.N_bps > 8) return DNRP_EUNSUPPORTED;
    const auto dm = geo::make_dims(*cfg, *psdef, q);
    const auto rs = geo::make_resampler(cfg->L, cfg->M, cfg->os_min, prm::RS_TX);
    if (S < dm.N_packet_rs) return DNRP_EINVAL;
    if (q.N_b_OCC + 1 > 1024) return DNRP_EUNSUPPORTED;
    uint32_t win_n = 0;
    const int werr = tx_window_n(dm, rs, win_fraction, &win_n);
    if (werr != DNRP_OK) return werr;
    const auto m = geo::build_maps(psdef->b, tm.N_TS, tm.N_eff_TX, q.N_DF_symb);
    const uint32_t ncb = geo::W_codebooks(tm.N_TS, tm.N_TX);
    std::vector<uint8_t> onehot(ncb);
    std::vector<dnrp_tx_desc> desc(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (codebook[i] >= ncb) return DNRP_EINVAL;
        desc[i].codebook_index = codebook[i];
    }
    for (uint32_t cb = 0; cb < ncb; ++cb) {
        float s = 1.0f;
        const auto W = geo::W_matrix(tm.N_TS, tm.N_TX, cb, &s);
        bool oh = true;
        for (uint32_t a = 0; a < tm.N_TX; ++a) {
            uint32_t nzc = 0;
            for (uint32_t ts = 0; ts < tm.N_TS; ++ts) nzc += W[size_t(a) * tm.N_TS + ts] != std::complex<float>(0.f, 0.f) ? 1u : 0u;
            oh = oh && nzc == 1;
        }
        onehot[cb] = oh ? 1 : 0;
    }
    // the streaming kernel's tables as tables.cpp get_tx builds them: the per-bin codes at 1024 points, the
    // one-hot codes where every spatial stream's symbol index fits the code word
    const uint64_t n_cells = m.pdc_sym_off.empty() ? 0 : m.pdc_sym_off.back();
    const bool code_bin = dm.Nd == 1024;
    const bool code_oh = code_bin && tm.N_TS > 1 && (tm.txdiv || n_cells == 0 || (n_cells - 1) * tm.N_SS + tm.N_TS - 1 <= dev::CODE_J_MASK);
    switches sw;
    read_tx(sw);
    dev::tx_args a{};
    plan_tx(tx_geom{&q, &tm, &dm, &rs, m.pdc_sym_off.data(), onehot.data(), code_bin, code_oh}, sw, n, desc.data(), S,
            (q.G + 7) / 8, uintptr_t(out_misalign), win_n, a);
    export_form(dev::tx_form_of(a, n), out);
    return DNRP_OK;
}

extern "C" int dnrp_ctx_set_tx_windowing(dnrp_ctx* ctx, float fraction) {
    if (!ctx || !(fraction >= 0.0f && fraction <= 1.0f)) return DNRP_EINVAL;  // NaN fails both comparisons
    ctx->tx_win_fraction = fraction;
    return DNRP_OK;
}

extern "C" int dnrp_tx_window(uint32_t N_b_DFT_os, float fraction, float* rising, uint32_t cap) {
    const uint32_t N = window_length(N_b_DFT_os, fraction);
    if (N == 0) return DNRP_EINVAL;
    if (!rising) return static_cast<int>(N);
    if (cap < N) return DNRP_EINVAL;
    const auto rc = window_rising(N);
    std::memcpy(rising, rc.data(), N * sizeof(float));
    return static_cast<int>(N);
}

extern "C" int dnrp_tx_batch(dnrp_ctx* ctx, const dnrp_psdef* psdef, uint32_t n, const dnrp_tx_desc* desc, const uint8_t* pcc_d,
                  const uint8_t* pdc_d, uint32_t pdc_stride, float* iq_out, uint32_t S, void* stream) {
    if (!ctx || !psdef || (n > 0 && (!desc || !pcc_d || !pdc_d || !iq_out))) return DNRP_EINVAL;
    if (n == 0) return DNRP_OK;
    if (n > ctx->cfg.max_batch) return DNRP_ENOMEM;
    (void)hipSetDevice(ctx->cfg.device);
    read_tx(ctx->sw);
    int err = DNRP_OK;
    tx_tables* t = get_tx(ctx, *psdef, &err);
    if (!t) return err;
    if (S < t->dm.N_packet_rs || pdc_stride < (t->q.G + 7) / 8) return DNRP_EINVAL;
    if (t->q.N_b_OCC + 1 > 1024) return DNRP_EUNSUPPORTED;
    // OFDM windowing (dnrp_ctx_set_tx_windowing): the packet's window, checked before anything is
    // queued -- the reference asserts 2 <= N (dft/windowing.cpp:39)
    uint32_t win_n = 0;
    const float* win = nullptr;
    err = tx_window_n(t->dm, t->rs, ctx->tx_win_fraction, &win_n);
    if (err != DNRP_OK) return err;
    if (win_n) {
        uint32_t fbits;
        std::memcpy(&fbits, &ctx->tx_win_fraction, sizeof fbits);
        auto& wb = ctx->tx_win[{t->dm.Nd, fbits}];
        if (!wb) {
            auto nb = std::make_unique<dbuf>();
            if (!nb->upload(window_rising(win_n))) return DNRP_ENOMEM;
            wb = std::move(nb);
        }
        win = wb->as<float>();
    }
    auto* pk = static_cast<dev::tx_pkt*>(ctx->st_tx.get(sizeof(dev::tx_pkt) * n));
    if (!pk) return DNRP_ENOMEM;
    for (uint32_t i = 0; i < n; ++i) {
        const auto& d = desc[i];
        if ((d.plcf_type != 1 && d.plcf_type != 2) || d.GI_percentage > 100) return DNRP_EINVAL;
        if (d.codebook_index >= t->wscale.size()) return DNRP_EINVAL;
        auto it = ctx->netid.find(d.network_id);
        if (it == ctx->netid.end()) return DNRP_ENETID;
        err = ensure_seq(ctx, *it->second, d.network_id, t->q.G);
        if (err != DNRP_OK) return err;
        pk[i].pdc_seq = (d.plcf_type == 1 ? it->second->t1 : it->second->t2).as<uint8_t>();
        pk[i].codebook = d.codebook_index;
        // tx.cpp:582-594: standard W scaling, or the dynamic-range optimised one
        const float sc = d.DAC_scale * (d.optimal_scaling_DAC ? t->wscale_opt[d.codebook_index] : t->wscale[d.codebook_index]);
        pk[i].scale_stf = 1.0f / std::sqrt(static_cast<float>(t->q.N_b_OCC / 4)) * sc;
        pk[i].scale_df = 1.0f / std::sqrt(static_cast<float>(t->q.N_b_OCC)) * sc;
        pk[i].ph0 = phasor_arg(d.iq_phase_rad);
        pk[i].inc = phasor_arg(d.iq_phase_increment_s2s_post_resampling_rad);
        pk[i].do_mix = (pk[i].ph0 != 0.0 || pk[i].inc != 0.0) ? 1u : 0u;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!ctx->tx_pk.ensure(sizeof(dev::tx_pkt) * ctx->cfg.max_batch)) return DNRP_ENOMEM;
    HIPCHK(ctx->tx_pk.wait_idle(st));
    HIPCHK(hipMemcpyAsync(ctx->tx_pk.p, pk, sizeof(dev::tx_pkt) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->st_tx.ev, st));
    dev::tx_args a{};
    plan_tx(tx_geom{&t->q, &t->tm, &t->dm, &t->rs, t->pdc_off_h.data(), t->w_onehot.data(), t->code_bin.p != nullptr,
                    t->code_oh.p != nullptr},
            ctx->sw, n, desc, S, pdc_stride, reinterpret_cast<uintptr_t>(iq_out), win_n, a);
    a.plan = t->plan;
    if (a.big_len) {
        // the DECT-rate scratch of the symbols (tx.hip tx_big_sym_kernel), big_batch packets per pass
        const uint64_t row_bytes = sizeof(float) * 2 * uint64_t(a.big_len) * t->tm.N_TX;
        if (!ctx->tx_big.ensure(row_bytes * a.big_batch)) return DNRP_ENOMEM;
        HIPCHK(ctx->tx_big.wait_idle(st));
        a.big = ctx->tx_big.as<float2>();
    }
    a.code = t->code.as<uint32_t>();
    a.pdc_off = t->pdc_off.as<uint32_t>();
    a.stf = t->stf.as<float2>();
    a.W = t->W.as<float2>();
    a.taps = t->taps.as<float>();
    a.taps_pp = t->taps_pp.as<float>();
    a.npp = t->npp;
    a.tw = t->tw.as<float2>();
    a.qam = t->qam.as<float2>();
    a.qpsk = t->qpsk.as<float2>();
    a.pcc_seq = ctx->pcc_seq.as<uint8_t>();
    a.pcc_d = pcc_d;
    a.pdc_d = pdc_d;
    a.out = iq_out;
    a.pk = ctx->tx_pk.as<dev::tx_pkt>();
    a.win = win;
    if (a.stream) {
        a.code_bin = t->code_bin.as<uint32_t>();
        a.code_oh = t->code_oh.as<uint32_t>();
        a.pcc_syms = t->pcc_syms;
    }
    ctx->tic("tx", st);
    if (dev::launch_tx(a, n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("tx", st);
    ctx->tx_form = dev::tx_form_of(a, n);  // dnrp_tx_last_form
    ctx->tx_form_valid = true;
    HIPCHK(ctx->tx_pk.mark_busy(st));
    if (a.big) HIPCHK(ctx->tx_big.mark_busy(st));
    return DNRP_OK;
}
