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

}  // namespace

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
    if (ctx->tx_win_fraction > 0.0f) {
        win_n = window_length(t->dm.Nd, ctx->tx_win_fraction);
        if (win_n == 0) return t->dm.Nd % 8 ? DNRP_EUNSUPPORTED : DNRP_EINVAL;
        // tx.hip tx_window_run leaves the prefix of a run's history symbol unshaped: the resampler
        // history must end behind it
        if (win_n > t->dm.CP || t->rs.hl + win_n >= t->dm.CP + t->dm.Nd) return DNRP_EUNSUPPORTED;
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
    a.plan = t->plan;
    a.N_occ = t->q.N_b_OCC;
    a.off_lower = t->dm.off_lower;
    a.CP = t->dm.CP;
    a.STF_CP = t->dm.STF_CP;
    a.N_DF = t->q.N_DF_symb;
    a.N_TS = t->tm.N_TS;
    a.N_TX = t->tm.N_TX;
    a.N_SS = t->tm.N_SS;
    a.N_bps = t->q.N_bps;
    a.txdiv = t->tm.txdiv;
    fill_pairs(t->tm.N_TS, a.pair, a.mod);
    a.pattern_len = t->dm.pattern_len;
    a.L = t->rs.L;
    a.M = t->rs.M;
    a.delay = t->rs.delay;
    a.hl = t->rs.hl;
    a.n_keep = std::min(t->dm.N_no_GI_rs, S);
    a.S = S;
    a.pdc_stride = pdc_stride;
    a.G = t->q.G;
    // symbol runs (tx.hip): K symbols per WG plus the preceding symbol as resampler history
    // wave path (one wavefront per symbol slot): K = 6 symbols + history per 7-wave workgroup
    // (C4, 4096 slots per launch: K=3 12.3 ms, K=4 16.6, K=5 15.2, K=6 11.4, K=7 15.9 — LDS sets
    // 4 / 2 / 2 / 2 / 1 workgroups per CU); block path K = 3.
    const bool wave = t->dm.Nd == 1024;
    const uint32_t K = wave ? 6u : 3u;
    a.K = K;
    a.n_runs = (t->q.N_DF_symb + 1 + K - 1) / K;
    const auto al = geo::resampler_align(t->rs);
    a.m_star = al.m_star;
    a.p_star = al.p_star;
    a.HP = 2 * (t->rs.hl + t->rs.M + 1);
    {
        const uint32_t len0 = t->dm.STF_CP + t->dm.Nd, lenD = t->dm.CP + t->dm.Nd;
        auto bsym = [&](uint32_t l) { return l == 0 ? 0u : len0 + (l - 1) * lenD; };
        const uint32_t bpc = t->tm.N_SS * t->q.N_bps;
        uint32_t mx = 0, span = 0;
        for (uint32_t r = 0; r < a.n_runs; ++r) {
            const uint32_t lf = r * K, ll = std::min(lf + K, t->q.N_DF_symb + 1) - 1, s0 = std::max(lf, 1u) - 1;
            span = std::max(span, bsym(ll + 1) - bsym(s0));
            const uint64_t b0 = (uint64_t(t->pdc_off_h[std::max(s0, 1u)]) * bpc) >> 3;
            const uint64_t b1 = ((uint64_t(t->pdc_off_h[ll + 1]) * bpc + 7) >> 3) + 1;
            if (b1 > b0) mx = std::max<uint32_t>(mx, static_cast<uint32_t>(b1 - b0));
        }
        a.stage_bytes = mx <= 8192 ? (mx + 3) / 4 * 4 : 0;
        a.lin_len = std::max(2 * a.HP + span, (K + 1) * t->dm.Nd);
        // output staging reuses bufB + twiddles + constellation: size bufB for the longest run
        const uint32_t max_out = static_cast<uint32_t>((uint64_t(span + t->rs.hl) * t->rs.L + t->rs.M - 1) / t->rs.M) + t->rs.L;
        a.bufB_len = std::max((K + 1) * t->dm.Nd, max_out > t->dm.Nd + 256 ? max_out - t->dm.Nd - 256 : 0u);
    }
    if (t->dm.Nd > 1024) {
        // beyond the block path's registers (tx_kernel stages <= 4 bins per thread): the symbols go
        // through a DECT-rate scratch (tx.hip tx_big_sym_kernel), e.g. u < u_max at b_max = 16
        const uint64_t total = uint64_t(t->dm.STF_CP) + uint64_t(t->q.N_DF_symb) * t->dm.CP + uint64_t(t->q.N_DF_symb + 1) * t->dm.Nd;
        a.big_len = static_cast<uint32_t>((total + 3) / 4 * 4);
        // the scratch is capped at 4 GiB (sw.tx_big_cap): larger batches run in passes of big_batch packets (tx.hip)
        const uint64_t row_bytes = sizeof(float) * 2 * uint64_t(a.big_len) * t->tm.N_TX;
        a.big_batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(n, ctx->sw.tx_big_cap / row_bytes)));
        if (!ctx->tx_big.ensure(row_bytes * a.big_batch)) return DNRP_ENOMEM;
        HIPCHK(ctx->tx_big.wait_idle(st));
        a.big = ctx->tx_big.as<float2>();
        a.stage_bytes = 0;
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
    a.win_n = win_n;
    // streaming kernel (tx.hip tx_stream_kernel) where its geometry holds (its windowed form holds a
    // window of up to CP = 128 samples)
    a.stream = 0;
    if (wave && t->code_bin.p && dev::tx_stream_taps_match(t->rs.h.data(), t->rs.h.size()) && a.L == 10 && a.M == 9 && a.hl == 22 && a.CP == 128 && a.STF_CP == 1280 &&
        a.pattern_len * 9 == a.STF_CP + 1024 && S % 2 == 0 && (reinterpret_cast<uintptr_t>(iq_out) & 15u) == 0) {
        // every symbol's PDC bytes (SFBC partners included) within its staging window: 1 KiB, spatial
        // multiplexing 4 KiB (tx.hip TXS_SBW_SM: its first KiB prefetched, the rest loaded per symbol)
        const uint32_t bpc = t->tm.N_SS * t->q.N_bps;
        const bool sm = t->tm.N_TS > 1 && !t->tm.txdiv;
        uint64_t span = 0;
        for (uint32_t l = 1; l <= t->q.N_DF_symb; ++l) {
            const uint64_t j0 = t->pdc_off_h[l] & ~1u, j1 = (uint64_t(t->pdc_off_h[l + 1]) + 1) & ~1ull;
            const uint64_t ab = ((j0 * bpc) >> 3) & ~15ull, hi = ((j1 * bpc + 7) >> 3) + 1;
            span = std::max(span, hi - ab);
        }
        const bool fits = span <= (sm ? 4096u : 1024u);
        a.sb_chunks = static_cast<uint32_t>((span + 1023) / 1024);
        const int qlo0 = -static_cast<int>((a.p_star + 8) / 9);
        const int64_t mfirst0 = int64_t(a.m_star) + 10 * qlo0;
        if (fits) {
            a.stream = 1;
            a.mfma = ctx->sw.tx_mfma;
            a.code_bin = t->code_bin.as<uint32_t>();
            a.onehot = t->tm.N_TS > 1 && t->code_oh.p ? 1u : 0u;  // transmit diversity or spatial multiplexing
            for (uint32_t i = 0; i < n && a.onehot; ++i)
                a.onehot = t->w_onehot[desc[i].codebook_index] ? 1u : 0u;
            a.code_oh = t->code_oh.as<uint32_t>();
            a.pcc_syms = t->pcc_syms;
            a.n_pieces = static_cast<uint32_t>((int64_t(a.n_keep) - mfirst0 + 1279) / 1280);
            // enough wavefronts for ~8 rounds of 16 per CU; each extra segment costs one history FFT
            const uint64_t per = uint64_t(n) * a.N_TX;
            uint32_t ns = static_cast<uint32_t>(std::min<uint64_t>((32768 + per - 1) / per, std::max(1u, a.n_pieces / 8)));
            a.n_seg = std::max(1u, ns);
            a.piece_per_seg = (a.n_pieces + a.n_seg - 1) / a.n_seg;
            a.n_seg = (a.n_pieces + a.piece_per_seg - 1) / a.piece_per_seg;
        }
    }
    ctx->tic("tx", st);
    if (dev::launch_tx(a, n, st) != hipSuccess) return DNRP_EDEVICE;
    ctx->toc("tx", st);
    HIPCHK(ctx->tx_pk.mark_busy(st));
    if (a.big) HIPCHK(ctx->tx_big.mark_busy(st));
    return DNRP_OK;
}
