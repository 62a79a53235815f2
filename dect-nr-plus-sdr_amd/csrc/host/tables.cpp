// Per-configuration device tables of the C-ABI context: lookup, validation, the geometry of geo::
// and the uploads (TX, RX PCC phase, RX PDC phase).
#include "ctx_internal.hpp"

using namespace dnrp;
using namespace dnrp::host;

namespace {

// OFDM symbol of every PCC cell (rx_cells_kernel reads the symbol per cell in both phases)
std::vector<uint16_t> pcc_cell_symbols(const geo::maps_t& m) {
    std::vector<uint16_t> sym(m.pcc_k.size());
    for (size_t s = 0; s + 1 < m.pcc_sym_off.size(); ++s)
        for (uint32_t j = m.pcc_sym_off[s]; j < m.pcc_sym_off[s + 1]; ++j) sym[j] = static_cast<uint16_t>(m.pcc_l[s]);
    return sym;
}

// SFBC pair union windows of full symbols (rx_lut::pair_w, the fused receiver): per LUT row, stream
// class and pair u on subcarriers 2u, 2u + 1 (DC skipped) eq_compute's mean weights 0.5f (lo + hi) per
// tap of the union window, in the same float arithmetic. Left empty (false is only an upload failure)
// when some union window has more than 4 taps (the low-SNR profiles).
bool pair_windows(const geo::lut_t& L, uint32_t N_occ, dbuf& pair_w, dbuf& pair_p) {
    const uint32_t Nf = N_occ + 1, half = N_occ / 2, np = half, n = L.n;
    std::vector<float4> pw4(size_t(L.T) * 4 * np);
    std::vector<uint32_t> pb(size_t(L.T) * 4 * np);
    for (uint32_t r = 0; r < L.T; ++r)
        for (uint32_t cl = 0; cl < 4; ++cl)
            for (uint32_t u = 0; u < np; ++u) {
                const uint32_t k0 = 2 * u + (2 * u >= half ? 1u : 0u), k1 = 2 * u + 1 + (2 * u + 1 >= half ? 1u : 0u);
                const uint32_t w0 = L.pilot_weight[(size_t(r) * 4 + cl) * Nf + k0];
                const uint32_t w1 = L.pilot_weight[(size_t(r) * 4 + cl) * Nf + k1];
                const uint32_t p0 = w0 & 0xFFFFu, p1 = w1 & 0xFFFFu;
                const bool up = p1 >= p0;
                const uint32_t sh = up ? p1 - p0 : p0 - p1;
                const uint32_t wl = (up ? w0 : w1) >> 16, wh = (up ? w1 : w0) >> 16;
                if (n + sh > 4) return true;
                float wv[4];
                for (uint32_t i = 0; i < 4; ++i) {
                    const float lo = i < n ? L.weights[size_t(wl) * n + i] : 0.f;
                    const float hi = i >= sh && i - sh < n ? L.weights[size_t(wh) * n + i - sh] : 0.f;
                    wv[i] = 0.5f * (lo + hi);
                }
                pw4[(size_t(r) * 4 + cl) * np + u] = make_float4(wv[0], wv[1], wv[2], wv[3]);
                pb[(size_t(r) * 4 + cl) * np + u] = up ? p0 : p1;
            }
    return pair_w.upload(pw4) && pair_p.upload(pb);
}

// MIMO report: the single-stream codebook (1, N) of the candidates rx_mimo_kernel tries, its scaling
// factors and first used row
bool mimo_codebook(uint32_t N, dbuf& W, dbuf& sc, uint32_t& ncb, uint32_t& A0) {
    static const uint32_t A_nonzero[9] = {0, 0, 2, 0, 12, 0, 0, 0, 0};  // beamforming_...mapping.hpp:110-119, N_TS = 1
    if (N < 2) return true;
    if (N != 2 && N != 4) {
        // no single-stream codebook for 8 antennas (W_t::get_W(1, 8) is the SISO entry, and
        // the reference's W_mat_single.at(tx) throws, estimator_mimo.cpp:160-200): no
        // candidates, so rx_mimo_kernel reports 0xFFFFFFFF ("no recommendation")
        ncb = 0;
        A0 = 0;
        return W.upload(std::vector<float2>{make_float2(0.f, 0.f)}) && sc.upload(std::vector<float>{0.f});
    }
    ncb = geo::W_codebooks(1, N);
    A0 = A_nonzero[N];
    std::vector<float2> w;
    std::vector<float> s;
    for (uint32_t cb = 0; cb < ncb; ++cb) {
        float f = 1.f;
        for (const auto& v : geo::W_matrix(1, N, cb, &f)) w.push_back(make_float2(v.real(), v.imag()));
        s.push_back(f);
    }
    return W.upload(w) && sc.upload(s);
}

// rx_mimo_detail_kernel: the codebooks (R, N_TS) of the ranks R = 1, 2, 4 that N_TS transmit streams and N_RX
// receive antennas carry, back to back. N_TS = 8 has none (W_t::get_W(1, 8) is the SISO entry, not taken)
bool mimo_sm_codebooks(uint32_t N_TS, uint32_t N_RX, rx2_tables* t) {
    std::vector<float2> w;
    std::vector<float> s;
    for (uint32_t slot = 0; slot < 3; ++slot) {
        const uint32_t R = 1u << slot;
        t->sm_woff[slot] = static_cast<uint32_t>(w.size());
        t->sm_cboff[slot] = static_cast<uint32_t>(s.size());
        t->sm_ncb[slot] = 0;
        if (R > std::min(N_TS, N_RX) || (N_TS != 1 && N_TS != 2 && N_TS != 4)) continue;
        const uint32_t ncb = geo::W_codebooks(R, N_TS);
        if (ncb > dev::RX_MIMO_MAX_CB) return false;
        t->sm_ncb[slot] = ncb;
        for (uint32_t cb = 0; cb < ncb; ++cb) {
            float f = 1.f;
            for (const auto& v : geo::W_matrix(R, N_TS, cb, &f)) w.push_back(make_float2(v.real(), v.imag()));
            s.push_back(f);
        }
    }
    if (w.empty()) {  // non-empty uploads; the counts stay 0
        w.push_back(make_float2(0.f, 0.f));
        s.push_back(0.f);
    }
    return t->Wsm.upload(w) && t->ssm.upload(s);
}

}  // namespace

namespace dnrp::host {

bool tx_pair_codes(std::vector<uint32_t>& code, uint32_t N_TS) {
    uint32_t pair[12], mod = 1;
    fill_pairs(N_TS, pair, mod);
    for (auto& c : code) {
        const uint32_t ty = c & dev::CODE_MASK;
        if (ty == dev::CODE_DRS) {  // DRS: the stream in the pair field too (one W-row read per bin)
            c |= (c & 7u) << dev::CODE_PAIR_SHIFT;
            continue;
        }
        if (ty != dev::CODE_PCC && ty != dev::CODE_PDC) continue;
        const uint32_t j = c & ~dev::CODE_MASK;
        if (j > dev::CODE_J_MASK) return false;
        c = ty | j | (pair[(j >> 1) % mod] << dev::CODE_PAIR_SHIFT);
    }
    return true;
}

std::vector<uint32_t> tx_code_bin(const std::vector<uint32_t>& code, uint32_t N, uint32_t off_lower, uint32_t N_DF) {
    const uint32_t Nf = N + 1;
    std::vector<uint32_t> cb(size_t(N_DF + 1) * 1024, 0u);
    for (uint32_t l = 0; l <= N_DF; ++l)
        for (uint32_t nn = 0; nn < 1024; ++nn) {
            uint32_t k = 0xFFFFFFFFu;
            if (nn <= N / 2) k = N / 2 + nn;
            else if (nn >= off_lower && nn < off_lower + N / 2) k = nn - off_lower;
            // bin nn = lane + 64 m of the kernel's layout at [m / 4][lane][m % 4]: one 16-B load
            // per lane fetches the codes of four of its bins
            const uint32_t ln = nn & 63u, m = nn >> 6;
            if (k != 0xFFFFFFFFu) cb[size_t(l) * 1024 + ((m >> 2) * 64 + ln) * 4 + (m & 3u)] = code[size_t(l) * Nf + k];
        }
    return cb;
}

// one-hot W rows: every bin's code resolved per antenna stream ts (tx.hip bin_oh, kernels.hpp OH_*):
// the pair tests, the SFBC partner and its sign flips, the cell's place in the staged bytes and the
// cell type itself become fields the kernel's two table reads take as they are (tx.hip bin_df
// TXS_TXDIV1 / TXS_SM1 restated). Empty: not built (one stream, or a stream symbol index past the
// code word of the pair-testing form, which dnrp_tx_form_for tests the same way).
std::vector<uint32_t> tx_code_oh(const std::vector<uint32_t>& cb, const uint32_t* pdc_off, uint32_t N_DF, uint32_t N_TS, uint32_t N_SS,
                                 uint32_t N_bps, bool txdiv) {
    if (N_TS < 2 || N_bps == 0 || N_bps > 8) return {};
    auto word = [](uint32_t bo, uint32_t sh, uint32_t wd, uint32_t k) {
        return (bo & ((1u << dev::OH_BO_BITS) - 1u)) | (sh << dev::OH_SH_SHIFT) | (wd << dev::OH_WD_SHIFT) | (k << dev::OH_K_SHIFT);
    };
    // the index bit of a constellation point's re / im sign (36.211 7.1: the first / second bit; BPSK
    // has one bit for both, its flipped points are slots of their own)
    const uint32_t kx = N_bps == 1 ? dev::OH_Q_BPSK_FX : 1u << (N_bps - 1);
    const uint32_t ky = N_bps == 1 ? dev::OH_Q_BPSK_FY : 1u << (N_bps - 2);
    std::vector<uint32_t> oh(size_t(N_TS) * cb.size(), 0u);
    for (uint32_t ts = 0; ts < N_TS; ++ts)
        for (size_t i = 0; i < cb.size(); ++i) {
            const uint32_t c = cb[i], ty = c & dev::CODE_MASK, j = c & dev::CODE_J_MASK;
            const uint32_t pr = (c >> dev::CODE_PAIR_SHIFT) & 0xFFu, l = static_cast<uint32_t>(i / 1024);
            const bool ua = (pr & 0xFu) == ts, ub = (pr >> 4) == ts;
            if (l == 0) {  // the STF row: bin_stf reads the type alone
                oh[size_t(ts) * cb.size() + i] = ty == dev::CODE_STF ? c : 0u;
                continue;
            }
            uint32_t o = word(dev::OH_ZB, 8, 8, dev::OH_Q_ZERO);
            // first staged byte of the symbol (tx.hip txs_wave::stage_base)
            const uint64_t ab = ((uint64_t(pdc_off[l] & ~1u) * N_SS * N_bps) >> 3) & ~15ull;
            auto pdc = [&](uint64_t js, uint32_t k) {  // PDC symbol js of the packet's stream
                const uint64_t bit = js * N_bps - 8 * ab;
                const uint32_t bo = static_cast<uint32_t>(std::min<uint64_t>(bit >> 3, dev::OH_ZB));  // in the window where the kernel runs (plan_tx)
                return word(bo, 16 - static_cast<uint32_t>(bit & 7u) - N_bps, N_bps, k);
            };
            if (ty == dev::CODE_DRS) {
                if (ua) o = word(dev::OH_ZB, 8, 8, dev::OH_Q_DRS + ((j & 8u) ? 1u : 0u));
            } else if (ty == dev::CODE_PDC && !txdiv) {  // spatial multiplexing: the stream's symbol
                const uint64_t js = uint64_t(j) * N_SS + ts;
                if (js > dev::CODE_J_MASK) return {};
                o = pdc(js, 0);
            } else if ((ty == dev::CODE_PDC || ty == dev::CODE_PCC) && (ua || ub)) {
                // SFBC: stream A maps symbol j, stream B the partner j ^ 1 with (-re, +im) for
                // even j, (+re, -im) for odd j (transmit_diversity_precoding.cpp:37-75)
                const uint32_t jp = j ^ (ua ? 0u : 1u);
                if (ty == dev::CODE_PDC) {
                    o = pdc(jp, ua ? 0u : ((j & 1u) ? ky : kx));
                } else {  // QPSK of PCC bits 2 jp, 2 jp + 1 of the wave's descrambled bytes
                    const uint32_t k = dev::OH_Q_QPSK ^ (ua ? 0u : ((j & 1u) ? 1u : 2u));
                    o = word(dev::OH_PCB + ((2 * jp) >> 3), 14 - ((2 * jp) & 7u), 2, k);
                }
            }
            oh[size_t(ts) * cb.size() + i] = o;
        }
    return oh;
}

tx_tables* get_tx(dnrp_ctx* ctx, const dnrp_psdef& d, int* err) {
    const auto key = std::make_tuple(d.u, d.b, d.PacketLengthType, d.PacketLength, d.tm_mode_index, d.mcs_index, d.Z);
    auto it = ctx->txt.find(key);
    if (it != ctx->txt.end()) return it->second.get();
    auto t = std::make_unique<tx_tables>();
    if (!geo::packet_sizes(d, t->q, &t->tm)) {
        *err = DNRP_ECONFIG;
        return nullptr;
    }
    const auto& c = ctx->cfg;
    if (d.u > c.u_max || d.b > c.b_max || t->q.N_TX > c.N_TX_max || t->q.N_bps > 8) {
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    t->dm = geo::make_dims(c, d, t->q);
    t->plan = make_plan(t->dm.Nd);
    t->rs = geo::make_resampler(c.L, c.M, c.os_min, prm::RS_TX);
    const auto m = geo::build_maps(d.b, t->tm.N_TS, t->tm.N_eff_TX, t->q.N_DF_symb);
    std::vector<float2> stf(m.Nf);
    for (uint32_t k = 0; k < m.Nf; ++k) stf[k] = make_float2(m.stf[k].real(), m.stf[k].imag());
    std::vector<float2> W;
    const uint32_t ncb = geo::W_codebooks(t->tm.N_TS, t->tm.N_TX);
    for (uint32_t cb = 0; cb < ncb; ++cb) {
        float s = 1.0f;
        for (const auto& w : geo::W_matrix(t->tm.N_TS, t->tm.N_TX, cb, &s)) W.push_back(make_float2(w.real(), w.imag()));
        t->wscale.push_back(s);
        t->wscale_opt.push_back(geo::W_scaling_optimal_DAC(t->tm.N_TS, t->tm.N_TX, cb));
        // one nonzero entry in every antenna row (tx.hip TXS_TXDIV1)
        bool oh = true;
        for (uint32_t a = 0; a < t->tm.N_TX; ++a) {
            uint32_t nzc = 0;
            for (uint32_t ts = 0; ts < t->tm.N_TS; ++ts) {
                const float2 w = W[(size_t(cb) * t->tm.N_TX + a) * t->tm.N_TS + ts];
                nzc += (w.x != 0.f || w.y != 0.f) ? 1u : 0u;
            }
            oh = oh && nzc == 1;
        }
        t->w_onehot.push_back(oh ? 1 : 0);
    }
    t->pdc_off_h = m.pdc_sym_off;
    // transmit diversity TS pair (A | B << 4) per PCC/PDC cell into the code words (kernels.hpp CODE_*)
    std::vector<uint32_t> code = m.code;
    if (!tx_pair_codes(code, t->tm.N_TS)) {
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    if (uint64_t(t->dm.N_packet_rs + 2 * t->rs.hl) * t->rs.L >= (1ull << 32)) {  // 32-bit output indexing
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    {
        // streaming TX kernel: cell code per FFT bin (tx.hip tx_wg::code layout, 0 for empty bins)
        const uint32_t N = t->q.N_b_OCC, Nf = N + 1, Nd = t->dm.Nd;
        if (Nd == 1024) {
            const std::vector<uint32_t> cb = tx_code_bin(code, N, t->dm.off_lower, t->q.N_DF_symb);
            for (uint32_t l = 0; l <= t->q.N_DF_symb; ++l)
                for (uint32_t k = 0; k < Nf; ++k)
                    if ((code[size_t(l) * Nf + k] & dev::CODE_MASK) == dev::CODE_PCC) {
                        if (l >= 32) {
                            *err = DNRP_EUNSUPPORTED;
                            return nullptr;
                        }
                        t->pcc_syms |= 1u << l;
                    }
            if (!t->code_bin.upload(cb)) {
                *err = DNRP_ENOMEM;
                return nullptr;
            }
            const std::vector<uint32_t> oh = tx_code_oh(cb, t->pdc_off_h.data(), t->q.N_DF_symb, t->tm.N_TS, t->tm.N_SS, t->q.N_bps, t->tm.txdiv);
            if (!oh.empty() && !t->code_oh.upload(oh)) {
                *err = DNRP_ENOMEM;
                return nullptr;
            }
        }
    }
    if (!t->code.upload(code) || !t->stf.upload(stf) || !t->pdc_off.upload(m.pdc_sym_off) || !t->W.upload(W) || !t->taps.upload(t->rs.h) || !t->taps_pp.upload(taps_polyphase(t->rs, &t->npp)) ||
        !t->tw.upload(twiddles(t->dm.Nd)) || !t->qam.upload(constellation(t->q.N_bps)) ||
        !t->qpsk.upload(constellation(2))) {
        *err = DNRP_ENOMEM;
        return nullptr;
    }
    auto* r = t.get();
    ctx->txt[key] = std::move(t);
    return r;
}

rx1_tables* get_rx1(dnrp_ctx* ctx, uint32_t u, uint32_t b, uint32_t N_eff_TX, int* err) {
    const auto key = std::make_tuple(u, b, N_eff_TX);
    auto it = ctx->rx1t.find(key);
    if (it != ctx->rx1t.end()) return it->second.get();
    const auto& c = ctx->cfg;
    if (!(N_eff_TX == 1 || N_eff_TX == 2 || N_eff_TX == 4)) {  // N_eff_TX = 8 PCC ps LUT, see DESIGN.md
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    if (u > c.u_max || b > c.b_max || N_eff_TX > c.N_TX_max) {
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    auto t = std::make_unique<rx1_tables>();
    t->u = u;
    t->b = b;
    t->N_eff_TX = N_eff_TX;
    const uint64_t rate = uint64_t(c.u_max) * c.b_max * 1728000ull * c.os_min;
    t->Nd = static_cast<uint32_t>(rate / (uint64_t(u) * 27000ull));
    t->N_occ = 56 * b;
    t->off_lower = 32 * b + (t->Nd - 64 * b) + 4 * b;
    t->CP = 8 * b * t->Nd / (64 * b);
    const uint32_t stf = u == 1 ? 112 * b : 144 * b;
    t->STF_CP = (stf - 64 * b) * t->Nd / (64 * b);
    t->n_pattern = u == 1 ? 7 : 9;
    t->pattern_len = 16 * b * t->Nd / (64 * b);
    t->plan = make_plan(t->Nd);
    t->rs = geo::make_resampler(c.M, c.L, c.os_min, prm::RS_RX_SYNCED);  // RX swaps L and M (rx_synced.cpp:65-73)
    t->maps = geo::build_maps(b, N_eff_TX, N_eff_TX, 20);
    std::vector<geo::op_t> pcc_ops, dummy;
    geo::build_rx_ops(t->maps, N_eff_TX, 20, c.chestim_mode_lr != 0, std::max(1u, c.chestim_lr_stride), pcc_ops, dummy,
                      t->pcc_max);
    std::vector<float2> stfv(t->maps.Nf);
    for (uint32_t k = 0; k < t->maps.Nf; ++k) stfv[k] = make_float2(t->maps.stf[k].real(), t->maps.stf[k].imag());
    const auto plan = geo::build_rx_plan(t->maps, pcc_ops, N_eff_TX);
    t->drs_arith = geo::drs_tables_arithmetic(t->maps);
    bool ok = t->stf.upload(stfv) && t->tw.upload(twiddles(t->Nd)) && t->taps.upload(t->rs.h) && t->taps_pp.upload(taps_polyphase(t->rs, &t->npp)) &&
              t->drs_k.upload(t->maps.drs_k) && t->drs_v.upload(t->maps.drs_v) && t->pcc_k.upload(t->maps.pcc_k) &&
              t->pcc_sym.upload(pcc_cell_symbols(t->maps)) &&
              t->bplan.upload(plan);
    const uint32_t Nsv = N_eff_TX <= 2 ? 5 : 10;
    for (uint32_t mode = 0; mode < 2 && ok; ++mode)
        for (uint32_t p = 0; p < 3 && ok; ++p) {
            const auto L = geo::build_lut(mode ? Nsv : 0, b, c.b_max, c.u_max, p);
            ok = t->lut_pw[mode][p].upload(L.pilot_weight) && t->lut_w[mode][p].upload(L.weights) &&
                 (N_eff_TX < 2 || pair_windows(L, t->N_occ, t->lut_pair_w[mode][p], t->lut_pair_p[mode][p]));
            t->lut_n[mode][p] = L.n;
            t->lut_nw[mode][p] = static_cast<uint32_t>(L.weights.size());
            // 16-B slots: the segment table behind both weight tables stays 16-B aligned in LDS
            t->wcap[mode] = std::max(t->wcap[mode], (t->lut_nw[mode][p] + 3u) & ~3u);
            ok = ok && L.n < (1u << 15);  // eq_work packs the tap count into 15 bits
            t->lut_T[mode] = L.T;
        }
    std::vector<dev::rx_lut> luts(6);
    for (uint32_t mode = 0; mode < 2; ++mode)
        for (uint32_t p = 0; p < 3; ++p)
            luts[mode * 3 + p] = {t->lut_pw[mode][p].as<uint32_t>(), t->lut_w[mode][p].as<float>(), t->lut_n[mode][p],
                                  t->lut_nw[mode][p], t->lut_pair_w[mode][p].as<float4>(), t->lut_pair_p[mode][p].as<uint32_t>()};
    if (!ok || !t->luts.upload(luts)) {
        *err = DNRP_ENOMEM;
        return nullptr;
    }
    // a geometry is rejected only when neither the chunked STF layout (rx.hip rx_stf_lds, used from
    // N_b_DFT_os = 8192) nor any rx_fft layout fits one CU's 160 KiB of LDS
    if (!dev::rx_front_fits(front_args(ctx, t.get(), nullptr, nullptr))) {
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    auto* r = t.get();
    ctx->rx1t[key] = std::move(t);
    return r;
}

rx2_tables* get_rx2(dnrp_ctx* ctx, const dnrp_psdef& d, int* err) {
    const auto key = std::make_tuple(d.u, d.b, d.PacketLengthType, d.PacketLength, d.tm_mode_index, d.mcs_index, d.Z);
    auto it = ctx->rx2t.find(key);
    if (it != ctx->rx2t.end()) return it->second.get();
    auto t = std::make_unique<rx2_tables>();
    geo::tm_t tm;
    if (!geo::packet_sizes(d, t->q, &tm)) {
        *err = DNRP_ECONFIG;
        return nullptr;
    }
    // rx_synced.cpp:1331-1333: spatial multiplexing (AxA MIMO) is a \todo in the reference receiver;
    // demodulated here by MMSE only when the context opted in (DNRP_RX_MODE_SM_MMSE)
    const bool sm = tm.N_SS > 1;
    if ((sm && !(ctx->rx_mode & DNRP_RX_MODE_SM_MMSE)) || (sm && (tm.N_SS != tm.N_eff_TX || tm.N_SS > 4 ||
                                                                 ctx->cfg.N_TX_max < tm.N_SS)) ||
        tm.N_eff_TX > 4 || t->q.N_bps > 8) {
        *err = DNRP_EUNSUPPORTED;
        return nullptr;
    }
    t->sm = sm;
    t->maps = geo::build_maps(d.b, tm.N_TS, tm.N_eff_TX, t->q.N_DF_symb);
    std::vector<geo::op_t> pcc_ops, pdc_ops;
    uint32_t pm;
    geo::build_rx_ops(t->maps, tm.N_eff_TX, t->q.N_DF_symb, ctx->cfg.chestim_mode_lr != 0,
                      std::max(1u, ctx->cfg.chestim_lr_stride), pcc_ops, pdc_ops, pm);
    const auto plan = geo::build_rx_plan(t->maps, pdc_ops, tm.N_eff_TX, !sm);
    std::vector<uint16_t> csym(t->maps.pdc_k.size());
    for (uint32_t l = 0; l <= t->q.N_DF_symb; ++l)
        for (uint32_t j = t->maps.pdc_sym_off[l]; j < t->maps.pdc_sym_off[l + 1]; ++j) csym[j] = static_cast<uint16_t>(l);
    if (!t->pdc_k.upload(t->maps.pdc_k) || !t->pdc_sym.upload(csym) || !t->bplan.upload(plan)) {
        *err = DNRP_ENOMEM;
        return nullptr;
    }
    // MIMO report (estimator_mimo.cpp:80-160): the wideband DRS cells and the single-stream codebooks
    static_assert(prm::RX_MIMO_WIDEBAND_CELLS == 4, "rx_mimo_kernel sums 4 wideband cells");
    t->N_TS = tm.N_eff_TX;
    const auto mc = geo::rx_mimo_cells(t->maps, plan, t->N_TS);
    // fused PDC receiver (kernels/rx_fused.hip) and epoch receiver (kernels/rx_epoch.hip): their symbol
    // tables, where the phase qualifies; otherwise the Y path runs
    static_assert(sizeof(geo::rx_fsym_t) == sizeof(dev::rx_fsym), "rx_fsym layout");
    const bool dops_ok = !sm && plan.dl.size() <= dev::RX_MAX_DOPS;
    auto fu = geo::rx_fused_syms(t->maps, plan, tm.N_eff_TX, pm);
    auto ep = geo::rx_epoch_syms(t->maps, plan, pm);
    t->fused_ok = dops_ok && fu.ok;
    t->drs_y = fu.drs_y;
    t->n_fsym = static_cast<uint32_t>(fu.fsym.size());
    t->n_drs_syms = static_cast<uint32_t>(fu.drs_syms.size());
    t->ep_ok = dops_ok && ep.ok;
    t->n_ep_drs = static_cast<uint32_t>(ep.drs.size());
    for (auto* v : {&fu.drs_syms, &ep.sym, &ep.drs})
        if (v->empty()) v->push_back(0);  // non-empty uploads; the counts stay 0
    bool up = t->mimo_cells.upload(mc.cells) && t->mimo_signs.upload(mc.signs) && t->mimo_zcells.upload(mc.zcells) &&
              mimo_codebook(t->N_TS, t->Wtx, t->stx, t->ncb_tx, t->A_tx) &&
              mimo_codebook(ctx->cfg.N_TX_max, t->Wrx, t->srx, t->ncb_rx, t->A_rx) &&
              t->ncb_tx <= dev::RX_MIMO_MAX_CB && t->ncb_rx <= dev::RX_MIMO_MAX_CB &&
              mimo_sm_codebooks(t->N_TS, ctx->cfg.N_TX_max, t.get());
    if (t->fused_ok) up = up && t->fsym.upload(fu.fsym) && t->drs_syms.upload(fu.drs_syms);
    if (t->ep_ok) up = up && t->ep_off.upload(ep.off) && t->ep_sym.upload(ep.sym) && t->ep_drs.upload(ep.drs);
    // the epoch receiver's plan with twin segments (same epochs and cells, so its symbol lists hold);
    // rx_cells_kernel keeps the plain plan
    if (t->ep_ok && ctx->sw.eq_twin) {
        const auto tplan = geo::build_rx_plan(t->maps, pdc_ops, tm.N_eff_TX, true, true);
        if (geo::rx_twin_plan_ok(t->maps, plan, tplan)) {
            up = up && t->eplan.upload(tplan);
            t->eplan_ok = t->eplan.cells_ok;
        }
    }
    if (!up) {
        *err = DNRP_ENOMEM;
        return nullptr;
    }
    auto* r = t.get();
    ctx->rx2t[key] = std::move(t);
    return r;
}

}  // namespace dnrp::host
